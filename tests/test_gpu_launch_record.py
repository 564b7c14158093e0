"""The launch record of the five solvers that share one persistent-grid launcher (csrc/solver_launch.hpp):
TrustRegionNewton, NewtonDescent, NelderMead, GradientDescent, ConjugatedGradientDescent.  What last_launch() and
last_arithmetic() report after a solve is written in that one place; every expected value below follows from the launch
arithmetic (segments of a wavefront = 64 / lanes_per_problem, workgroups = ceil(B / segments) under the resident grid),
none from a measurement."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
B, N, LANES = 20, 3, 8
SOLVERS = ["BatchedTrustRegionNewton", "BatchedNewtonDescent", "BatchedNelderMead", "BatchedGradientDescent",
           "BatchedConjugatedGradientDescent"]
NO_LDS = ("BatchedGradientDescent", "BatchedConjugatedGradientDescent")   # x, g, d in registers, no per-problem LDS


@pytest.fixture
def context(monkeypatch, gpu_solver_factory):
    """context(cap): a fresh context whose resident grid is capped to `cap` workgroups (None: uncapped), through the
    variable the work-queue tests use.  (gpu_solver_factory first: the session's shared context is never made under it.)"""
    import cppnumericalsolvers_amd as amd
    made = []

    def make(cap=None):
        if cap is None:
            monkeypatch.delenv(CAP_ENV, raising=False)
        else:
            monkeypatch.setenv(CAP_ENV, str(cap))
        ctx = amd.Context(0)
        monkeypatch.delenv(CAP_ENV, raising=False)
        made.append(ctx)
        return ctx

    yield make
    for ctx in made:
        ctx.close()


def _starts(n):
    rng = np.random.default_rng(20261019)
    return np.ascontiguousarray(rng.uniform(-1.5, 1.5, size=(B, n)))


def _solver(name, ctx, **kw):
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    stop = capi.default_stop()
    stop.num_iterations = 25          # (the record does not depend on how far the solves get)
    return getattr(amd, name)(stopping_progress=stop, context=ctx, **kw)


def _solve(solver, x0):
    import torch
    import cppnumericalsolvers_amd as amd
    x, f, g, p = solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to("cuda:0"))
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


@pytest.mark.parametrize("name", SOLVERS)
def test_launch_record_of_twenty_problems_on_eight_lanes(context, name):
    solver = _solver(name, context(), lanes_per_problem=LANES)
    _solve(solver, _starts(N))
    ll = solver.last_launch()
    print(name, ll, solver.last_arithmetic())
    assert ll["lanes_per_problem"] == LANES and ll["elems_per_lane"] == 1, ll
    assert ll["threads"] == 64, ll
    assert ll["kernel"] == "general", ll
    assert solver.last_arithmetic() == "exact"
    # 64 / 8 = 8 segments per wavefront: ceil(20 / 8) = 3 workgroups, far below the resident grid
    assert ll["blocks"] == 3, ll
    if name in NO_LDS:
        assert ll["lds_bytes"] == 0, ll
    else:
        assert ll["lds_bytes"] > 0, ll


def test_gradient_descent_default_mapping_at_n_100(context):
    """n = 100 is above 64 lanes at one coordinate each: the library's choice is 64 lanes at two."""
    solver = _solver("BatchedGradientDescent", context())
    _solve(solver, _starts(100))
    ll = solver.last_launch()
    assert ll["lanes_per_problem"] == 64 and ll["elems_per_lane"] == 2, ll


@pytest.mark.parametrize("name", SOLVERS)
def test_capped_grid_is_recorded_and_changes_no_bit(context, name):
    x0 = _starts(N)
    free = _solver(name, context(), lanes_per_problem=LANES)
    want = _solve(free, x0)
    assert free.last_launch()["blocks"] == 3
    capped = _solver(name, context(1), lanes_per_problem=LANES)
    got = _solve(capped, x0)
    assert capped.last_launch()["blocks"] == 1, capped.last_launch()
    for a, b, what in zip(want, got, ("x", "f", "g", "progress")):
        assert a.tobytes() == b.tobytes(), (name, what)
