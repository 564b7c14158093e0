"""Every iterate of a device L-BFGS-B solve against the textbook definition of the step that produced it
(tests/bstep_lib.py: the generalized Cauchy point and the subspace step from the dense B at 200 bits), on the inputs of
tests/bstep_cases.py.  The same bound and the same two caps as the CPU twins in tests/test_bstep_lib.py; nothing here is
compared with a twin, and the device enters no calibration.

One launch per case with an amd.Trace of 8 of the 24 problems (3 at n = 100, 200).  Every row asserts that the kernel it
meant to run is the one that ran (last_launch(), last_arithmetic()).
"""
import time

import numpy as np
import pytest

import bstep_cases as Bc
import bstep_lib as Bs
from test_gpu_steps_mpmath import _dev, _stop, _start_values

pytestmark = pytest.mark.gpu
LINES = []
WORST = {}
ITERATION_LIMIT, GRADIENT = 1, 4          # Status of solver/progress.h


@pytest.fixture(scope="module", autouse=True)
def _lines_to_the_terminal_summary():
    yield
    import conftest
    for family, (total, slowest) in WORST.items():
        LINES.append("L-BFGS-B step audit, device %s: %s; slowest case %.1f s" % (family, total.line(), slowest))
    conftest._SUMMARY_LINES.extend(LINES)


@pytest.fixture(scope="module")
def ctx(gpu_solver_factory):
    return gpu_solver_factory().ctx


def _objective(name, blob):
    import cppnumericalsolvers_amd as amd
    return amd.Rosenbrock() if name == "rosenbrock" else amd.DiagQuadratic(blob[:-1], blob[-1])


def _lanes(n, m, arithmetic):
    """(lanes per problem, coordinates per lane) of the library's mapping of an L-BFGS-B shape"""
    if n > 128 or m > 8:
        lanes = 32
    else:
        lanes = 16
    E = 1
    while lanes * E < n:
        E *= 2
    return lanes, (8 if n > 64 else E)


def _solve(ctx, name, n, m, own, arithmetic, ran, linesearch="more_thuente", traced=Bc.TRACED, gradient_norm=None):
    """one traced launch -> (trajectories, lower, upper of the traced rows, status of the traced rows)"""
    import torch
    import cppnumericalsolvers_amd as amd
    blob, lower, upper, x0 = Bc.case(name, n, m, own)
    fields = Bc.stop_fields(Bc.limit(m)) if gradient_norm is None else Bc.stop_fields(Bc.limit(m), gradient_norm)
    solver = amd.BatchedLbfgsb(m=m, stopping_progress=_stop(fields), context=ctx, arithmetic=arithmetic, linesearch=linesearch)
    if own:
        solver.SetBoundsPerProblem(lower, upper)
    else:
        solver.SetBounds(lower[0], upper[0])
    rows = list(traced)
    trace = amd.Trace(rows, capacity=Bc.limit(m) + 2, n=n, device=solver.device, with_x=True, with_g=True)
    objective = _objective(name, blob)
    _, _, _, p = solver.minimize(objective, _dev(x0), trace=trace)
    torch.cuda.synchronize()
    assert solver.last_arithmetic() == ran
    launch = solver.last_launch()
    assert (launch["lanes_per_problem"], launch["elems_per_lane"]) == _lanes(n, m, ran), launch
    f0, g0 = _start_values(solver, objective, x0[rows])
    import step_cases
    trajectories = step_cases.trace_trajectories(trace, x0[rows], f0, g0)
    return trajectories, lower[rows], upper[rows], amd.progress_to_numpy(p)["status"][rows]


def _case(ctx, family, name, n, m, own, arithmetic, ran, **kw):
    started = time.perf_counter()
    trajectories, lower, upper, _ = _solve(ctx, name, n, m, own, arithmetic, ran, **kw)
    rules = lambda i: Bc.rules("relaxed" if ran == "fma" else "exact", m, lower[i], upper[i], kw.get("linesearch", "more_thuente"))
    rep = Bs.audit_case(trajectories, rules, what="%s %s n=%d m=%d" % (family, name, n, m))
    line = "%s %s n=%d m=%d %s: %s" % (family, name, n, m, "own boxes" if own else "shared box", rep.line())
    print(line)
    assert not rep.bad, "%s\n%d outside their bound, first: %s" % (line, len(rep.bad), rep.bad[:3])
    broken = Bs.caps(rep, m)
    assert not broken, "%s\n%s\nundecidable: %s" % (line, broken, rep.undecidable[:4])
    total, slowest = WORST.get(family, (Bs.Report(), 0.0))
    total.merge(rep)
    WORST[family] = (total, max(slowest, time.perf_counter() - started))
    return rep


# (objective, n, m, one box per problem): rows of tests/bstep_cases.py, on which the reference-order twin runs every branch
EXACT_ROWS = (("rosenbrock", 7, 3, True), ("rosenbrock", 17, 5, True), ("diag_quadratic", 17, 8, False),
              ("rosenbrock", 33, 5, True), ("rosenbrock", 64, 8, False), ("rosenbrock", 64, 8, True))
EXACT_WIDE_ROWS = (("diag_quadratic", 17, 10, False), ("rosenbrock", 33, 10, False))
RELAXED_ROWS = (("rosenbrock", 7, 3, True), ("rosenbrock", 9, 3, False), ("diag_quadratic", 17, 8, False),
                ("rosenbrock", 17, 5, True), ("diag_quadratic", 33, 10, False), ("rosenbrock", 33, 10, False),
                ("diag_quadratic", 64, 3, False), ("rosenbrock", 64, 8, False))


@pytest.mark.parametrize("name,n,m,own", EXACT_ROWS)
def test_reference_order_kernel_steps(ctx, name, n, m, own):
    """16 lanes; 1, 2, 4 coordinates per lane; capacity 5 and 8; a shared box and one box per problem"""
    _case(ctx, "reference-order kernel", name, n, m, own, "exact", "exact")


@pytest.mark.parametrize("name,n,m,own", EXACT_WIDE_ROWS)
def test_reference_order_kernel_steps_with_ten_pairs(ctx, name, n, m, own):
    """32 lanes per problem: m = 10"""
    _case(ctx, "reference-order kernel, 32 lanes", name, n, m, own, "exact", "exact")


@pytest.mark.parametrize("name,n,m,own", Bc.E8_ROWS)
def test_reference_order_kernel_steps_with_eight_coordinates_per_lane(ctx, name, n, m, own):
    """n = 100 on 16 lanes, n = 200 on 32; three traced problems"""
    _case(ctx, "reference-order kernel, 8 per lane", name, n, m, own, "exact", "exact", traced=Bc.E8_TRACED)


@pytest.mark.parametrize("name,n,m,own", RELAXED_ROWS)
def test_relaxed_kernel_steps(ctx, name, n, m, own):
    """the relaxed kernel, held to the bound the reference fixed: 1, 2, 4 coordinates per lane, capacity 5, 8 and 10, the
    staged form (n = 64), the own-box units"""
    _case(ctx, "relaxed kernel", name, n, m, own, "fma", "fma")


def test_default_arithmetic_runs_the_relaxed_kernel(ctx):
    _case(ctx, "relaxed kernel", "diag_quadratic", 9, 3, True, "default", "fma")


@pytest.mark.parametrize("name,n,m,own", [("rosenbrock", 9, 3, False), ("diag_quadratic", 17, 8, False)])
def test_hager_zhang_steps(ctx, name, n, m, own):
    """lbfgsb_solve_kernel<..., HagerZhang> at m <= 5, and one unit of the capacity-8 build (a shared box: one box per
    problem is built for the More-Thuente search)"""
    _case(ctx, "reference-order kernel, Hager-Zhang", name, n, m, own, "exact", "exact", linesearch="hager_zhang")


@pytest.mark.parametrize("arithmetic,name,n,m,own", [("exact", "rosenbrock", 17, 5, True), ("fma", "rosenbrock", 17, 5, True),
                                                     ("exact", "rosenbrock", 33, 10, False)])
def test_projected_gradient_stop_reads_the_previous_iterate(ctx, arithmetic, name, n, m, own):
    """`ProjectedGradientInfNorm` is a maximum of doubles, with no rounding: the solve ends with the gradient status at
    iteration k iff the norm at iterate k - 1 is the first below the (absolute) tolerance"""
    tolerance = 1e-2
    trajectories, lower, upper, status = _solve(ctx, name, n, m, own, arithmetic, arithmetic, gradient_norm=tolerance)
    ended = 0
    for i, (xs, gs, _) in enumerate(trajectories):
        T = len(xs) - 1
        norms = [np.max(np.abs(np.where(((xs[k] <= lower[i]) & (gs[k] > 0)) | ((xs[k] >= upper[i]) & (gs[k] < 0)), 0.0, gs[k])))
                 for k in range(T + 1)]
        below = [k for k in range(T) if norms[k] < tolerance]
        if status[i] == GRADIENT:
            assert below == [T - 1], (i, T, norms)
            ended += 1
        else:
            assert status[i] == ITERATION_LIMIT and not below, (i, T, status[i], norms)
    assert ended > 0


def test_ask_tell_box_handle_steps(ctx):
    """n = 33, m = 5: the trajectory is what the caller sees between two tells; the objective is numpy Rosenbrock on the
    host copies of the device arrays (pinned to its definition by tests/hp_lib.py's bounds in tests/test_step_lib.py)"""
    import torch
    import cppnumericalsolvers_amd as amd
    name, n, m, own = "rosenbrock", 33, 5, True
    _, lower, upper, x0 = Bc.case(name, n, m, own)

    def fun(x):
        t1, t2 = 1.0 - x[:, :-1], x[:, 1:] - x[:, :-1] * x[:, :-1]
        g = np.zeros_like(x)
        g[:, :-1] += -2.0 * t1 - 400.0 * x[:, :-1] * t2
        g[:, 1:] += 200.0 * t2
        return np.sum(t1 * t1 + 100.0 * t2 * t2, axis=1), g

    box = amd.BatchedLbfgsb(m=m, stopping_progress=_stop(Bc.stop_fields(Bc.limit(m))), context=ctx, arithmetic="exact")
    box.SetBoundsPerProblem(lower, upper)
    at = amd.LbfgsbAskTell(box, _dev(x0))
    rows = list(Bc.TRACED)
    f0, g0 = fun(x0)
    out = [([x0[b]], [g0[b]], [f0[b]]) for b in rows]
    seen = [0] * len(rows)
    for _ in range(40 * (Bc.limit(m) + 2)):
        f, g = fun(at.x.cpu().numpy())
        active = at.tell(_dev(f), _dev(g))
        x, fv, gv, p = at.results()
        torch.cuda.synchronize()
        x, fv, gv, p = x.cpu().numpy(), fv.cpu().numpy(), gv.cpu().numpy(), amd.progress_to_numpy(p)
        for i, b in enumerate(rows):
            if p["num_iterations"][b] > seen[i]:
                assert p["num_iterations"][b] == seen[i] + 1
                seen[i] += 1
                out[i][0].append(x[b])
                out[i][1].append(gv[b])
                out[i][2].append(fv[b])
        if active == 0:
            break
    at.close()
    assert active == 0
    trajectories = [(np.array(xs), np.array(gs), np.array(fs)) for xs, gs, fs in out]
    rep = Bs.audit_case(trajectories, lambda i: Bc.rules("exact", m, lower[rows[i]], upper[rows[i]]), what="ask/tell box handle")
    line = "L-BFGS-B step audit, device ask/tell box handle n=%d m=%d: %s" % (n, m, rep.line())
    assert not rep.bad, "%s\n%s" % (line, rep.bad[:3])
    assert not Bs.caps(rep, m), "%s\n%s" % (line, rep.undecidable[:4])
    LINES.append(line)
