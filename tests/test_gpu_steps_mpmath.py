"""Every iterate of a device solve against the textbook definition of the step that produced it (tests/step_lib.py), on the
rows of tests/step_cases.py: the direction H_k g_k from the dense matrix update at 200 bits, the line-search conditions on the
device's own numbers, the traced value and gradient of every iterate against the definitions of tests/hp_lib.py.  The same
bounds and the same two caps as the CPU twins in tests/test_step_lib.py; nothing here is compared with a twin.

One launch per case with an amd.Trace of 8 of the 24 problems; the entries that refuse a trace (float32, n > 256) and the
lean kernels, which a trace would switch off, take one small launch of the 8 problems per iteration.
"""
import os

import numpy as np
import pytest

import step_cases as Sc
import step_lib as St

pytestmark = pytest.mark.gpu
LINES = []
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _lines_to_the_terminal_summary():
    yield
    import conftest
    conftest._SUMMARY_LINES.extend(LINES)


@pytest.fixture(scope="module")
def ctx(gpu_solver_factory):
    return gpu_solver_factory().ctx


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _stop(fields):
    from cppnumericalsolvers_amd import capi
    s = capi.Stop()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _objective(name, blob):
    import cppnumericalsolvers_amd as amd
    if name == "rosenbrock":
        return amd.Rosenbrock()
    if name == "rosenbrock_second":
        return amd.Rosenbrock("second")
    obj = amd.DiagQuadratic(blob[:-1], blob[-1])
    if name == "diag_quadratic_second":
        obj.hessian_diagonal = np.ascontiguousarray(2.0 * blob[:-1])     # the constant diagonal of its Hessian
    return obj


def _start_values(solver, objective, x0):
    """the device's own f(x_0), g(x_0).  The evaluation entry ends at n = 256; above it (chained Rosenbrock only) the
    gradient, which has no sum in it, comes from two overlapping windows of 256 coordinates — coordinate j from a window
    that holds j - 1 and j + 1 — and the value as the sum of the terms below 255 and of those from 255 on (one more
    rounding than the kernel's: that row's audit of the value starts at iterate 1)."""
    import torch
    n = x0.shape[1]
    if n > 256:
        assert objective.name == "rosenbrock" and n < 510
        (fa, ga), (_, gb), (fc, _) = [_start_values(solver, objective, part)
                                      for part in (x0[:, :256], x0[:, n - 256:], x0[:, 255:])]
        return fa + fc, np.concatenate([ga[:, :255], gb[:, 255 - (n - 256):]], axis=1)
    f0, g0 = solver.evaluate(objective, _dev(x0))
    torch.cuda.synchronize()
    return f0.cpu().numpy(), g0.cpu().numpy()


def _traced(make_solver, objective, x0, m, after_launch=None):
    """one launch of the whole batch with a trace of the rows TRACED"""
    import torch
    import cppnumericalsolvers_amd as amd
    solver = make_solver(_stop(Sc.stop_fields(Sc.limit(m))))
    rows = list(Sc.TRACED)
    trace = amd.Trace(rows, capacity=Sc.limit(m) + 2, n=x0.shape[1], device=solver.device, with_x=True, with_g=True)
    solver.minimize(objective, _dev(x0), trace=trace)
    torch.cuda.synchronize()
    if after_launch:
        after_launch(solver)
    f0, g0 = _start_values(solver, objective, x0[rows])
    return Sc.trace_trajectories(trace, x0[rows], f0, g0)


def _prefix_limited(make_solver, objective, x0, m, after_launch=None):
    """iterate k from the launch limited to k - 1 iterations, the 8 traced problems per launch"""
    import torch
    import cppnumericalsolvers_amd as amd
    rows = x0[list(Sc.TRACED)]

    def solve(part, fields):
        solver = make_solver(_stop(fields))
        x, f, g, p = solver.minimize(objective, _dev(part))
        torch.cuda.synchronize()
        if after_launch:
            after_launch(solver)
        return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)

    f0, g0 = _start_values(make_solver(_stop(Sc.stop_fields(1))), objective, rows)
    return Sc.prefix_trajectories(solve, rows, f0, g0, m)


def _finish(title, reports):
    total = St.Report()
    for m, what, rep in reports:
        Sc.assert_case(rep, m, what)
        total.merge(rep)
    LINES.append("step audit, device %s: %s" % (title, total.line()))


def _lbfgs_case(ctx, family, name, start, n, m, W=0, E=0, placement=0, linesearch="more_thuente"):
    import cppnumericalsolvers_amd as amd
    blob, evaluate, ks = Sc.objective(name, n)
    objective = _objective(name, blob)
    x0 = Sc.starts(start, n)
    make = lambda stop: amd.BatchedLbfgs(m=m, stopping_progress=stop, context=ctx, arithmetic=family, lanes_per_problem=W,
                                         elems_per_lane=E, history_placement=placement, linesearch=linesearch)

    def ran(solver):
        assert solver.last_arithmetic() == family
        if W:
            ll = solver.last_launch()
            assert (ll["lanes_per_problem"], ll["elems_per_lane"]) == (W, E)

    trajectories = (_prefix_limited if n > 256 else _traced)(make, objective, x0, m, after_launch=ran)
    rules = Sc.rules_of(family, m, linesearch=linesearch, second=name.endswith("_second"))
    return Sc.audit_once(trajectories, rules, evaluate, ks, Sc.hess_diag(name, n), first_value=1 if n > 256 else 0,
                         what="%s %s %s n=%d m=%d %dx%d placement %d" % (family, name, start, n, m, W, E, placement))


@pytest.mark.parametrize("family,name,start,n,m",
                         Sc.lbfgs_rows(("exact", "fma"), extra=(("diag_quadratic_second", "std", 7, 3),)))
def test_lbfgs_steps_are_the_textbook_steps(ctx, family, name, start, n, m):
    """the library's own mapping of every shape, exact and fused; n = 300 the workgroup kernel (exact arithmetic)"""
    rep = _lbfgs_case(ctx, family, name, start, n, m)
    _finish("%s n=%d" % (family, n), [(m, "%s %s %s n=%d m=%d" % (family, name, start, n, m), rep)])


@pytest.mark.parametrize("name,start,n,m", Sc.MAPPING_SHAPES)
def test_every_built_mapping_and_both_history_placements(ctx, name, start, n, m):
    """every built (lanes, coordinates per lane) that covers n, two and four coordinates per lane among them, with the
    history in LDS and with its y half in registers; fused arithmetic (the exact kernels are one tree on every mapping)"""
    reports = []
    for W, E in Sc.mappings_of(n):
        for placement in Sc.PLACEMENTS:
            reports.append((m, "fma %dx%d placement %d %s n=%d m=%d" % (W, E, placement, name, n, m),
                            _lbfgs_case(ctx, "fma", name, start, n, m, W=W, E=E, placement=placement)))
    assert reports
    _finish("fma, every mapping, both placements, n=%d" % n, reports)


@pytest.mark.parametrize("family", ["exact", "fma"])
@pytest.mark.parametrize("name,start,n,m", Sc.HZ_SHAPES)
def test_hager_zhang_steps(ctx, family, name, start, n, m):
    rep = _lbfgs_case(ctx, family, name, start, n, m, linesearch="hager_zhang")
    _finish("%s hager_zhang n=%d" % (family, n), [(m, "%s hager_zhang %s n=%d m=%d" % (family, name, n, m), rep)])


def test_lean_kernel_steps(ctx):
    """Rosenbrock-32, m = 6, the default arithmetic, no plateau ring, no trace: every launch runs the lean kernel"""
    import cppnumericalsolvers_amd as amd
    name, start, n, m = Sc.LEAN_SHAPE
    _, evaluate, ks = Sc.objective(name, n)
    make = lambda stop: amd.BatchedLbfgs(m=m, stopping_progress=stop, context=ctx, arithmetic="default")
    kernels = []
    trajectories = _prefix_limited(make, amd.Rosenbrock(), Sc.starts(start, n), m,
                                   after_launch=lambda s: kernels.append(s.last_launch()["kernel"]))
    assert kernels and set(kernels) == {"lean"}, kernels
    rep = St.audit_case(trajectories, Sc.rules_of("fma", m), evaluate, ks, what="lean rosenbrock n=%d m=%d" % (n, m))
    _finish("lean n=%d" % n, [(m, "lean rosenbrock n=%d m=%d" % (n, m), rep)])


@pytest.mark.parametrize("name,start,n,m", Sc.F32_SHAPES)
def test_float32_steps(ctx, name, start, n, m):
    import torch
    import cppnumericalsolvers_amd as amd
    blob, evaluate, ks = Sc.objective(name, n, "float32")
    make = lambda stop: amd.BatchedLbfgs(m=m, stopping_progress=stop, context=ctx, arithmetic="exact", dtype=torch.float32)
    trajectories = _prefix_limited(make, _objective(name, blob), Sc.starts(start, n, "float32"), m)
    rep = St.audit_case(trajectories, Sc.rules_of("f32", m, dtype="float32"), evaluate, ks,
                        what="float32 %s %s n=%d m=%d" % (name, start, n, m))
    _finish("float32 n=%d" % n, [(m, "float32 %s %s n=%d m=%d" % (name, start, n, m), rep)])


@pytest.mark.parametrize("name,start,n", Sc.BFGS_SHAPES)
def test_dense_bfgs_steps(ctx, name, start, n):
    import cppnumericalsolvers_amd as amd
    m = Sc.BFGS_M
    blob, evaluate, ks = Sc.objective(name, n)
    make = lambda stop: amd.BatchedBfgs(stopping_progress=stop, context=ctx)
    trajectories = _traced(make, _objective(name, blob), Sc.starts(start, n), m)
    rep = St.audit_case(trajectories, Sc.rules_of("bfgs", m, solver="bfgs"), evaluate, ks,
                        what="bfgs %s %s n=%d" % (name, start, n))
    _finish("bfgs n=%d" % n, [(m, "bfgs %s %s n=%d" % (name, start, n), rep)])


@pytest.mark.parametrize("arithmetic", ["exact", "default"])
@pytest.mark.parametrize("per_problem", [False, True])
@pytest.mark.parametrize("name,start,n,m", Sc.LBFGSB_SHAPES)
def test_lbfgsb_keeps_the_box_and_the_decrease(ctx, name, start, n, m, per_problem, arithmetic):
    """the reduced check: the box holds exactly at every iterate, and every step that reaches no bound meets the first
    line-search inequality; the reference-order kernels and the relaxed default, a shared box and one box per problem,
    starts on a bound"""
    import cppnumericalsolvers_amd as amd
    blob, evaluate, ks = Sc.objective(name, n)
    lower, upper = Sc.box(n, per_problem)
    x0 = Sc.box_starts(start, n, lower, upper)

    def make(stop):
        s = amd.BatchedLbfgsb(m=m, stopping_progress=stop, context=ctx, arithmetic=arithmetic)
        (s.SetBoundsPerProblem if per_problem else s.SetBounds)(lower, upper)
        return s

    trajectories = _traced(make, _objective(name, blob), x0, m)
    total = St.Report()
    for i, b in enumerate(Sc.TRACED):
        lo, hi = (lower[b], upper[b]) if per_problem else (lower, upper)
        total.merge(St.audit_case(trajectories[i:i + 1], Sc.rules_of("lbfgsb", m, solver="lbfgsb", lower=lo, upper=hi),
                                  evaluate, ks, what="lbfgsb %s n=%d problem %d" % (arithmetic, n, b)))
    label = "lbfgsb %s %s n=%d" % (arithmetic, "own boxes" if per_problem else "shared box", n)
    _finish(label, [(m, label, total)])


@pytest.mark.parametrize("n,m", Sc.DENSE_QUARTIC_SHAPES)
def test_dense_quartic_functor_steps(n, m):
    """the dense quartic example functor (objective 101 of the library built with it): direction and line search, and the
    traced value and gradient of every iterate against hp_lib.dense_quartic"""
    import cppnumericalsolvers_amd as amd
    import hp_lib
    params, x0 = Sc.dense_quartic(n)
    S, b, kappa = params[:n * n].reshape(n, n).T, params[n * n:n * n + n], params[-1]
    evaluate = lambda x: hp_lib.dense_quartic(x, S, b, kappa)
    user = amd.Context(0, library=os.path.join(REPO, "cppnumericalsolvers_amd", "libmi355_lbfgs_tr.so"))
    try:
        make = lambda stop: amd.BatchedLbfgs(m=m, stopping_progress=stop, context=user, arithmetic="exact")
        trajectories = _traced(make, amd.Objective(101, params, "dense_quartic"), x0, m)
    finally:
        user.close()
    rep = St.audit_case(trajectories, Sc.rules_of("exact", m), evaluate, hp_lib.dense_quartic_k(n)[:2],
                        what="dense quartic n=%d m=%d" % (n, m))
    _finish("dense quartic n=%d" % n, [(m, "dense quartic n=%d m=%d" % (n, m), rep)])
