"""The device objective functors against their plain definitions at 200 bits (tests/hp_lib.py), under the rounding bounds
derived there — no CPU twin takes part.  Every built (lanes_per_problem, elems_per_lane) that covers n, every input family
of tests/hp_cases.py in one call per (mapping, n); the definitions are evaluated once per (objective, n) and shared by the
mappings.  Where the magnitude of a value is 0 the device value must be exactly 0.

The matrix-core ridge form and the composite objective of AugLagComposite have solve entry points only: they are pinned
through a solve that stops after its first iteration, which returns the functor's value and gradient at the x it
returns, and the composite also through the augmented-Lagrangian solver's evaluation entry.
"""
import numpy as np
import pytest

import hp_cases as Cs
import hp_lib as hp
from test_gpu_fma import MAPPINGS as FMA_MAPPINGS
from test_gpu_parity import MAPPINGS as EXACT_MAPPINGS

pytestmark = pytest.mark.gpu
REPORTS = Cs.Reports()


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios_to_the_terminal_summary():
    """one line per title, appended to conftest._SUMMARY_LINES when the module's last test has run"""
    yield
    REPORTS.append_to_summary()


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(*tensors):
    _torch().cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def _finish(worst, title, bad):
    REPORTS.report(title, worst)
    assert not bad, "%d values outside their bound, first: %s" % (len(bad), bad[:3])


def _audit_rows(refs, f, g, ks, worst, label, what, dtype="float64", H=None):
    bad = []
    for b, ev in enumerate(refs):
        bad += Cs.audit(ev, f[b], g[b], ks, dtype=dtype, H=None if H is None else H[b].T, worst=worst, label=label,
                        what="%s %s" % (what, Cs.FAMILIES[b]))
    return bad


@pytest.mark.parametrize("arithmetic", ["exact", "fma"])
@pytest.mark.parametrize("n", Cs.DIMS)
def test_rosenbrock_and_diag_quadratic_against_the_definition(gpu_solver_factory, n, arithmetic):
    import cppnumericalsolvers_amd as amd
    X = _dev(Cs.inputs(n))
    a, c = Cs.diag_coefficients(n)
    worst, bad, ran = Cs.Worst(), [], 0
    for W, E in (EXACT_MAPPINGS if arithmetic == "exact" else FMA_MAPPINGS):
        if W * E < n:
            continue
        s = gpu_solver_factory(lanes_per_problem=W, elems_per_lane=E, arithmetic=arithmetic)
        for name, objective, refs, ks in (("rosenbrock", amd.Rosenbrock(), Cs.rosenbrock_reference(n), hp.rosenbrock_k(n)),
                                         ("diag_quadratic", amd.DiagQuadratic(a, c), Cs.diag_quadratic_reference(n),
                                          hp.diag_quadratic_k(n))):
            f, g = _host(*s.evaluate(objective, X))
            bad += _audit_rows(refs, f, g, ks, worst, name + " ", "%s %s n=%d (%d, %d)" % (name, arithmetic, n, W, E))
        ran += 1
    assert ran > 0
    _finish(worst, "mpmath bound, device fp64 %s (error / bound)" % arithmetic, bad)


def _float_mappings(n):
    """the library's own mapping and the wider ones the float path builds (tests/test_gpu_lbfgs_f32.py)"""
    import l32_lib
    W, E = l32_lib.library_mapping(n)
    return [(0, 0)] + [(w, 1) for w in (16, 32, 64) if w > W and E == 1] + ([(64, 4)] if (W, E) == (64, 2) else [])


@pytest.mark.parametrize("n", Cs.DIMS)
def test_float_objectives_against_the_definition(gpu_solver_factory, n):
    import cppnumericalsolvers_amd as amd
    torch = _torch()
    X = _dev(Cs.inputs(n, "float32"))
    a, c = Cs.diag_coefficients(n, "float32")
    worst, bad = Cs.Worst(), []
    for W, E in _float_mappings(n):
        s = amd.BatchedLbfgs(m=6, context=gpu_solver_factory().ctx, arithmetic="exact", dtype=torch.float32,
                             lanes_per_problem=W, elems_per_lane=E)
        for name, objective, refs, ks in (
                ("rosenbrock", amd.Rosenbrock(), Cs.rosenbrock_reference(n, "float32"), hp.rosenbrock_k(n)),
                ("diag_quadratic", amd.DiagQuadratic(a, c), Cs.diag_quadratic_reference(n, "float32"),
                 hp.diag_quadratic_k(n))):
            f, g = _host(*s.evaluate(objective, X))
            assert f.dtype == np.float32 and g.dtype == np.float32
            bad += _audit_rows(refs, f, g, ks, worst, name + " ", "%s float32 n=%d (%d, %d)" % (name, n, W, E),
                               dtype="float32")
    _finish(worst, "mpmath bound, device float32 (error / bound)", bad)


@pytest.mark.parametrize("n", Cs.DIMS)
def test_derivative_checker_outputs_against_the_definition(gpu_solver_factory, n):
    """f, grad and hess of amd.check_derivatives; hess is column major, [b, j, i] = H(i, j) (n <= 64: the Hessian kernels
    hold one coordinate per lane; above, value and gradient)."""
    import cppnumericalsolvers_amd as amd
    X = _dev(Cs.inputs(n))
    a, c = Cs.diag_coefficients(n)
    hessian = n <= 64
    worst, bad = Cs.Worst(), []
    for lanes in ((0, 64) if n <= 32 else (0,)):   # (the library's own mapping, and a wider one where it is narrower)
        for name, objective, refs, ks in (
                ("rosenbrock", amd.Rosenbrock(), Cs.rosenbrock_reference(n, hessian=hessian), hp.rosenbrock_k(n)),
                ("diag_quadratic", amd.DiagQuadratic(a, c), Cs.diag_quadratic_reference(n, hessian=hessian),
                 hp.diag_quadratic_k(n))):
            r = amd.check_derivatives(objective, X, hessian=hessian, lanes_per_problem=lanes,
                                      context=gpu_solver_factory().ctx)
            f, g = _host(r.f, r.grad)
            H = _host(r.hess)[0] if hessian else None
            bad += _audit_rows(refs, f, g, ks, worst, name + " ", "%s derivatives n=%d lanes=%d" % (name, n, lanes), H=H)
    _finish(worst, "mpmath bound, device derivative check (error / bound)", bad)


def _one_iteration():
    from cppnumericalsolvers_amd import capi
    s = capi.default_stop()
    s.num_iterations = 1
    return s


def _audit_at_returned_x(evaluate, x, f, g, ks, worst, label, what):
    """f and g a solve returned are the definition's at the x it returned"""
    bad = []
    for b in range(x.shape[0]):
        assert np.isfinite(x[b]).all() and np.isfinite(f[b]) and np.isfinite(g[b]).all(), (what, b)
        bad += Cs.audit(evaluate(b, x[b]), f[b], g[b], ks, worst=worst, label=label, what="%s %s" % (what, Cs.FAMILIES[b]))
    return bad


@pytest.mark.parametrize("rows,n", Cs.RIDGE_SHAPES + Cs.RIDGE_GRAM_SHAPES)
def test_ridge_forms_against_the_definition(gpu_solver_factory, rows, n):
    """One definition, four device forms: the VALU form on every mapping its LDS copy of A fits, the two normal-equation
    forms (shared matrix, one matrix per problem), and the matrix-core form through a one-iteration solve."""
    import cppnumericalsolvers_amd as amd
    A, Y, X = Cs.ridge_data(rows, n)
    R, refs = Cs.ridge_reference(rows, n)
    worst, bad = Cs.Worst(), []
    s = gpu_solver_factory(m=10, arithmetic="default")
    f, g = _host(*s.evaluate(amd.SquaredErrorRidge(A, Cs.RIDGE_LAMBDA, gram=True), _dev(X), per_problem=_dev(Y)))
    bad += _audit_rows(refs, f, g, R.k(), worst, "gram ", "ridge gram (%d, %d)" % (rows, n))
    As, Yo, Xo = Cs.ridge_own_data(rows, n)
    f, g = _host(*s.evaluate(amd.SquaredErrorRidgePerProblem(rows, Cs.RIDGE_LAMBDA), _dev(Xo),
                             per_problem=_dev(amd.ridge_per_problem_rows(As, Yo))))
    bad += _audit_rows(Cs.ridge_own_reference(rows, n), f, g, (n + rows, n + rows), worst, "own ",
                       "ridge own (%d, %d)" % (rows, n))
    if (rows, n) in Cs.RIDGE_SHAPES:
        for W, E in EXACT_MAPPINGS:
            if n <= W * E <= 128:
                sv = gpu_solver_factory(lanes_per_problem=W, elems_per_lane=E)
                f, g = _host(*sv.evaluate(amd.SquaredErrorRidge(A, Cs.RIDGE_LAMBDA), _dev(X), per_problem=_dev(Y)))
                bad += _audit_rows(refs, f, g, R.k(), worst, "valu ", "ridge valu (%d, %d) (%d, %d)" % (rows, n, W, E))
        for arithmetic in ("exact", "fma"):
            sm = gpu_solver_factory(m=10, stopping_progress=_one_iteration(), arithmetic=arithmetic)
            x, f, g = _host(*sm.minimize(amd.SquaredErrorRidge(A, Cs.RIDGE_LAMBDA, matrix_cores=True), _dev(X),
                                         per_problem=_dev(Y))[:3])
            bad += _audit_at_returned_x(lambda b, xb: R(xb, Y[b]), x, f, g, R.k(), worst, "mfma ",
                                        "ridge mfma %s (%d, %d)" % (arithmetic, rows, n))
    _finish(worst, "mpmath bound, device ridge forms (error / bound)", bad)


def _engine_problem(n, terms, n_eq):
    from cppnumericalsolvers_amd import ConstrainedProblem
    mk = lambda t: ConstrainedProblem.term([(p[0], p[1], p[2]) for p in t[0]], t[1], t[2], product=t[3])
    return ConstrainedProblem(n, mk(terms[0]), [mk(t) for t in terms[1:1 + n_eq]], [mk(t) for t in terms[1 + n_eq:]])


COMPOSITE_COUNTS = ((0, 0), (1, 0), (0, 1), (2, 2), (4, 0), (0, 4), (3, 1), (4, 4))


@pytest.mark.parametrize("n", Cs.COMPOSITE_DIMS)
def test_composite_against_the_definition(gpu_solver_factory, n):
    """0 ... 4 constraints of each kind over every kind, form, sum and product of the menu; row 0 of every case with an
    inequality sits within 1e-12 of the kink of its max(0, .).  The solver's evaluation entry, and AugLagComposite with
    per-problem rows (lambda, mu, rho) under a BatchedLbfgs solve of one iteration."""
    import cppnumericalsolvers_amd as amd
    ctx = gpu_solver_factory().ctx
    worst, bad = Cs.Worst(), []
    for n_eq, n_ineq in COMPOSITE_COUNTS:
        terms, X, lam, mu, rho = Cs.composite_case(n, n_eq, n_ineq)
        k = hp.composite_k(n, terms)
        problem = _engine_problem(n, terms, n_eq)
        what = "composite n=%d eq=%d ineq=%d" % (n, n_eq, n_ineq)
        f, g = amd.BatchedAugmentedLagrangian(context=ctx).evaluate_host(problem, X, lam, mu, rho)
        bad += _audit_rows(Cs.composite_reference(n, n_eq, n_ineq), f, g, (k, k), worst, "evaluation ", what)
        rows = np.hstack([lam, mu, rho[:, None]])
        s = gpu_solver_factory(m=10, stopping_progress=_one_iteration())
        x, f, g = _host(*s.minimize(amd.AugLagComposite(problem), _dev(X), per_problem=_dev(rows))[:3])
        bad += _audit_at_returned_x(lambda b, xb: hp.composite(xb, terms, n_eq, lam[b], mu[b], rho[b]), x, f, g, (k, k),
                                    worst, "solve ", what + " after one iteration")
    _finish(worst, "mpmath bound, device composite (error / bound)", bad)
