"""What the solvers RETURN, audited without a twin: postconditions that hold for any correct solver (tests/hp_cases.py,
audit_results), with the objective's value and gradient taken from tests/hp_lib.py at 200 bits at the exact x returned.
Small batches (24 problems) from the seeds of tests/at_lib.py's starts, no hostile rows, under the default and the parity
stop.  tests/test_hp_lib.py runs the same audit on the CPU twins and shows that these starts end on no bail-out.
"""
import numpy as np
import pytest

import hp_cases as Cs

pytestmark = pytest.mark.gpu
REPORTS = Cs.Reports()


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios_to_the_terminal_summary():
    """one line per title, appended to conftest._SUMMARY_LINES when the module's last test has run"""
    yield
    REPORTS.append_to_summary()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _solve(solver, objective, x0, **kw):
    import torch
    import cppnumericalsolvers_amd as amd
    x, f, g, p = solver.minimize(objective, _dev(x0), **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


def _finish(worst, title, bad):
    REPORTS.report(title, worst)
    assert not bad, "%d postconditions broken, first: %s" % (len(bad), bad[:3])


def _stops(preset="default"):
    import cppnumericalsolvers_amd as amd
    return (("default", amd.capi.default_stop(preset)), ("parity", amd.parity_stop()))


def _objective(name, params):
    import cppnumericalsolvers_amd as amd
    return amd.Rosenbrock() if name == "rosenbrock" else amd.DiagQuadratic(params[0], params[1])


def _solvers(ctx, stop, lbfgsb_stop, n):
    """(label, solver, keyword arguments of the audit, dtype) of every solver of the unconstrained tests"""
    import torch
    import cppnumericalsolvers_amd as amd
    box, boxes = Cs.result_box(n), Cs.result_box(n, per_problem=True)
    out = [("lbfgs exact", amd.BatchedLbfgs(m=10, stopping_progress=stop, context=ctx, arithmetic="exact"), {}),
           ("lbfgs fma", amd.BatchedLbfgs(m=10, stopping_progress=stop, context=ctx, arithmetic="fma"), {}),
           ("lbfgs hager_zhang", amd.BatchedLbfgs(m=10, stopping_progress=stop, context=ctx, arithmetic="exact",
                                                  linesearch="hager_zhang"), {}),
           ("lbfgs float32", amd.BatchedLbfgs(m=6, stopping_progress=stop, context=ctx, arithmetic="exact",
                                              dtype=torch.float32), dict(dtype="float32")),
           ("bfgs", amd.BatchedBfgs(stopping_progress=stop, context=ctx), {}),
           ("trust_region", amd.BatchedTrustRegionNewton(stopping_progress=stop, context=ctx), {}),
           ("newton_descent", amd.BatchedNewtonDescent(stopping_progress=stop, context=ctx), {}),
           ("gradient_descent", amd.BatchedGradientDescent(stopping_progress=stop, context=ctx), {}),
           ("conjugated_gradient_descent", amd.BatchedConjugatedGradientDescent(stopping_progress=stop, context=ctx), {}),
           ("nelder_mead", amd.BatchedNelderMead(stopping_progress=stop, context=ctx), dict(value_only=True))]
    for arithmetic in ("exact", "default"):      # the reference-order kernels and the relaxed default
        shared = amd.BatchedLbfgsb(m=5, stopping_progress=lbfgsb_stop, context=ctx, arithmetic=arithmetic)
        shared.SetBounds(*box)
        own = amd.BatchedLbfgsb(m=5, stopping_progress=lbfgsb_stop, context=ctx, arithmetic=arithmetic)
        own.SetBoundsPerProblem(*boxes)
        out += [("lbfgsb %s shared box" % arithmetic, shared, dict(lower=box[0], upper=box[1], lbfgsb=True)),
                ("lbfgsb %s own boxes" % arithmetic, own, dict(lower=boxes[0], upper=boxes[1], lbfgsb=True))]
    return out


@pytest.mark.parametrize("n", Cs.RESULT_DIMS)
@pytest.mark.parametrize("name", ["rosenbrock", "diag_quadratic"])
def test_every_solver_returns_what_it_reports(gpu_solver_factory, name, n):
    ctx = gpu_solver_factory().ctx
    worst, bad = Cs.Worst(), []
    for (stop_name, stop), (_, lbfgsb_stop) in zip(_stops(), _stops("lbfgsb")):
        for label, solver, kw in _solvers(ctx, stop, lbfgsb_stop, n):
            dtype = kw.get("dtype", "float64")
            params, evaluate, ks, minimiser, mu = Cs.result_objective(name, n, dtype)
            x0 = Cs.result_starts(name, n).astype(np.float32 if dtype == "float32" else np.float64)
            if kw.get("lbfgsb"):
                x0 = np.clip(x0, kw["lower"], kw["upper"])
            elif minimiser is not None and not kw.get("value_only"):
                kw = dict(kw, minimiser=minimiser, mu=mu)
            x, f, g, p = _solve(solver, _objective(name, params), x0)
            b, _ = Cs.audit_results(evaluate, ks, x0, x, f, g, p, solver.stopping_progress, worst=worst, label=label + " ",
                                    what="%s n=%d %s %s" % (name, n, label, stop_name), **kw)
            bad += b
    _finish(worst, "mpmath bound, returned f and g, %s (error / bound)" % name, bad)


def test_lean_and_wide_kernels_return_what_they_report(gpu_solver_factory):
    """arithmetic="default" on Rosenbrock-32 with m = 6 runs the lean launch-specialised kernel; n = 300 the workgroup
    kernel for n > 256."""
    import cppnumericalsolvers_amd as amd
    ctx = gpu_solver_factory().ctx
    worst, bad = Cs.Worst(), []
    for stop_name, stop in _stops():
        for n, m, kernel in ((32, 6, "lean"), (300, 10, None)):
            _, evaluate, ks, _, _ = Cs.result_objective("rosenbrock", n)
            x0 = Cs.result_starts("rosenbrock", n)
            s = amd.BatchedLbfgs(m=m, stopping_progress=stop, context=ctx, arithmetic="default")
            x, f, g, p = _solve(s, amd.Rosenbrock(), x0)
            if kernel is not None:   # (the lean kernel is built for stops without the plateau ring: the parity stop)
                assert s.last_launch()["kernel"] == (kernel if stop.past == 0 else "general")
            else:
                assert s.last_launch()["threads"] == 256
            b, _ = Cs.audit_results(evaluate, ks, x0, x, f, g, p, stop, worst=worst, label="n=%d " % n,
                                    what="rosenbrock n=%d %s" % (n, stop_name))
            bad += b
    _finish(worst, "mpmath bound, returned f and g, lean and wide kernels (error / bound)", bad)


@pytest.mark.parametrize("rows,n", Cs.RIDGE_RESULT_SHAPES)
def test_ridge_forms_return_what_they_report(gpu_solver_factory, rows, n):
    """The four forms; the strongly convex inequality with x* from a 200-bit LU and mu = 2 lam (the own-matrix form: a
    batch of 8 with one LU per problem and no bail-out allowed)."""
    import cppnumericalsolvers_amd as amd
    ctx = gpu_solver_factory().ctx
    A, Y, x0, evaluate, ks, minimiser, mu = Cs.ridge_result_case(rows, n)
    As, Yo, x0o, evaluate_own, ks_own, minimiser_own, mu_own = Cs.ridge_own_result_case(rows, n)
    worst, bad = Cs.Worst(), []
    for stop_name, stop in _stops():
        forms = [("valu", "exact", amd.SquaredErrorRidge(A, Cs.RIDGE_LAMBDA)),
                 ("mfma", "default", amd.SquaredErrorRidge(A, Cs.RIDGE_LAMBDA, matrix_cores=True)),
                 ("gram", "default", amd.SquaredErrorRidge(A, Cs.RIDGE_LAMBDA, gram=True))]
        for label, arithmetic, objective in forms:
            s = amd.BatchedLbfgs(m=10, stopping_progress=stop, context=ctx, arithmetic=arithmetic)
            x, f, g, p = _solve(s, objective, x0, per_problem=_dev(Y))
            b, _ = Cs.audit_results(evaluate, ks, x0, x, f, g, p, stop, minimiser=minimiser, mu=mu, worst=worst,
                                    label=label + " ", what="ridge %s (%d, %d) %s" % (label, rows, n, stop_name))
            bad += b
        s = amd.BatchedLbfgs(m=10, stopping_progress=stop, context=ctx, arithmetic="default")
        x, f, g, p = _solve(s, amd.SquaredErrorRidgePerProblem(rows, Cs.RIDGE_LAMBDA), x0o,
                            per_problem=_dev(amd.ridge_per_problem_rows(As, Yo)))
        b, _ = Cs.audit_results(evaluate_own, ks_own, x0o, x, f, g, p, stop, minimiser=minimiser_own, mu=mu_own,
                                worst=worst, label="own ", what="ridge own (%d, %d) %s" % (rows, n, stop_name))
        bad += b
    _finish(worst, "mpmath bound, returned f and g, ridge forms (error / bound)", bad)


def _engine_problem(n, terms, n_eq):
    from cppnumericalsolvers_amd import ConstrainedProblem
    mk = lambda t: ConstrainedProblem.term([(p[0], p[1], p[2]) for p in t[0]], t[1], t[2], product=t[3])
    return ConstrainedProblem(n, mk(terms[0]), [mk(t) for t in terms[1:1 + n_eq]], [mk(t) for t in terms[1 + n_eq:]])


@pytest.mark.parametrize("n", Cs.RESULT_DIMS)
def test_composite_under_lbfgs_returns_what_it_reports(gpu_solver_factory, n):
    """AugLagComposite(problem) with per-problem rows (lambda, mu, rho) as the objective of BatchedLbfgs."""
    import cppnumericalsolvers_amd as amd
    ctx = gpu_solver_factory().ctx
    terms, n_eq, x0, lam, mu, rho, evaluate, k = Cs.composite_result_case(n)
    worst, bad = Cs.Worst(), []
    for stop_name, stop in _stops():
        s = amd.BatchedLbfgs(m=10, stopping_progress=stop, context=ctx, arithmetic="exact")
        x, f, g, p = _solve(s, amd.AugLagComposite(_engine_problem(n, terms, n_eq)), x0,
                            per_problem=_dev(np.hstack([lam, mu, rho[:, None]])))
        b, _ = Cs.audit_results(evaluate, (k, k), x0, x, f, g, p, stop, worst=worst, label="composite ",
                                what="composite n=%d %s" % (n, stop_name))
        bad += b
    _finish(worst, "mpmath bound, returned f and g, composite (error / bound)", bad)


def test_augmented_lagrangian_reports_its_violation_and_kkt_norm(gpu_solver_factory):
    """max_violation and the KKT norm BatchedAugmentedLagrangian returns, against their definitions at the returned x and
    multipliers (tests/hp_cases.py, audit_al_report)."""
    import cppnumericalsolvers_amd as amd
    worst, bad = Cs.Worst(), []
    for n, n_eq, n_ineq in Cs.AL_REPORT_CASES:
        terms, x0 = Cs.al_report_case(n, n_eq, n_ineq)
        s = amd.BatchedAugmentedLagrangian(context=gpu_solver_factory().ctx)
        s.config = s.default_config(outer_num_iterations=30)
        d = s.minimize_host(_engine_problem(n, terms, n_eq), x0)
        bad += Cs.audit_al_report(terms, n_eq, d["x"], d["lambda"], d["mu"], d["max_violation"],
                                  d["max_lagrangian_gradient"], worst=worst, what="n=%d" % n)
    _finish(worst, "mpmath bound, augmented-Lagrangian report (error / bound)", bad)
