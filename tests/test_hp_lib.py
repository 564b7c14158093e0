"""tests/hp_lib.py on the CPU: the definitions check themselves against mp.diff, the CPU twins (which the GPU suite holds
bitwise equal to the device) stay inside the derived rounding bounds on every input family and shape of
tests/test_gpu_objectives_mpmath.py, and wrong kernels built from hp_lib's own pieces do not.

Worst error-to-bound ratios go to the terminal summary (conftest._SUMMARY_LINES) and are copied into DESIGN.md section 5.
"""
import numpy as np
import pytest

import hp_cases as Cs
import hp_lib as hp

mp, mpf = hp.mp, hp.mpf
DIFF_TOL = mpf(10) ** -40
REPORTS = Cs.Reports()


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios_to_the_terminal_summary():
    """one line per title, appended to conftest._SUMMARY_LINES when the module's last test has run"""
    yield
    REPORTS.append_to_summary()


def _width(n):
    return 1 << max(3, int(np.ceil(np.log2(n))))


# ---- 1. the definitions check themselves ----------------------------------------------------------------------------------
def _close(got, want, scale):
    """1e-40 relative; an entry that is structurally zero is compared on the scale of the function's other entries"""
    return abs(got - want) <= DIFF_TOL * (abs(want) if want != 0 else scale)


def _unit(n, j):
    return tuple(1 if i == j else 0 for i in range(n))


def _self_check(evaluate, points, hessian):
    """evaluate(list of mpf) -> (f, g, H) at 200 bits.  g and H against mp.diff of f alone."""
    for x in points:
        n = len(x)
        f, g, H = evaluate(x)
        fx = lambda *args: evaluate(list(args))[0]
        scale = max(abs(v) for v in g)
        for j in range(n):
            assert _close(g[j], mp.diff(fx, tuple(x), _unit(n, j)), scale), ("g", j)
        if hessian:
            for i in range(n):
                for j in range(n):
                    order = tuple(a + b for a, b in zip(_unit(n, i), _unit(n, j)))
                    assert _close(H[i][j], mp.diff(fx, tuple(x), order), scale), ("H", i, j)


def _points(n, seed):
    rng = np.random.default_rng(seed)
    return [hp.vec(rng.uniform(-2.0, 2.0, n)), hp.vec(1.0 + 0.1 * rng.normal(size=n)), hp.vec(3.0 * rng.normal(size=n))]


def test_rosenbrock_derivatives_are_the_derivatives_of_its_value():
    for n in (1, 2, 5):
        _self_check(lambda x: hp._rosenbrock(hp._PLAIN, x, hessian=True), _points(n, n), hessian=True)


def test_diag_quadratic_derivatives_are_the_derivatives_of_its_value():
    for n in (1, 4):
        a, c = Cs.diag_coefficients(n)
        _self_check(lambda x: hp._diag_quadratic(hp._PLAIN, x, hp.vec(a), mpf(c), hessian=True), _points(n, 10 + n),
                    hessian=True)


def test_ridge_gradient_is_the_derivative_of_its_value():
    rng = np.random.default_rng(5)
    for rows, n in ((5, 3), (2, 4)):
        R = hp.Ridge(rng.normal(size=(rows, n)), 0.3)
        y = hp.vec(rng.normal(size=rows))
        _self_check(lambda x: R._eval(hp._PLAIN, R.A, R.AT, x, y), _points(n, rows), hessian=False)


def test_ridge_minimiser_is_the_solution_of_mp_lu_solve():
    rng = np.random.default_rng(11)
    for rows, n in ((9, 5), (4, 7)):
        R = hp.Ridge(rng.normal(size=(rows, n)), 0.1)
        G = mp.matrix([[mp.fdot(R.AT[i], R.AT[j]) + (R.lam if i == j else 0) for j in range(n)] for i in range(n)])
        for _ in range(2):     # (the second right-hand side reuses the factors)
            y = rng.normal(size=rows)
            want = mp.lu_solve(G, mp.matrix([mp.fdot(R.AT[j], hp.vec(y)) for j in range(n)]))
            assert all(abs(a - b) <= DIFF_TOL * abs(b) for a, b in zip(R.minimiser(y), want))


def test_composite_gradient_is_the_derivative_of_its_value():
    """Every kind, form, sum and product of the menu, with inequalities on both sides of their max(0, .)."""
    n, n_eq, n_ineq = 3, 4, 4
    terms = [hp._mpf_term(hp._PLAIN, t) for t in Cs.composite_terms(n, n_eq, n_ineq)]
    lam, rho = hp.vec([0.7, -0.4, 0.2, -1.1]), mpf(1.75)
    sides = set()
    for mu in (hp.vec([0.3, 1.9, 0.0, 2.5]), hp.vec([40.0, 0.1, 30.0, 0.0])):
        for x in _points(n, 3) + [hp.vec([0.2, -0.1, 0.15])]:   # (the last: inside the ball of the first inequality)
            for q in range(n_ineq):
                sides.add((q, hp._term(hp._PLAIN, terms[1 + n_eq + q], x)[0] * rho < mu[q]))
            _self_check(lambda z: hp._composite(hp._PLAIN, z, terms, n_eq, lam, mu, rho), [x], hessian=False)
    assert len(sides) == 2 * n_ineq, "every inequality was seen active and inactive"


# ---- 2. the twins meet the bounds -------------------------------------------------------------------------------------------
def _rows(oracle, objective, X, **kw):
    return [oracle.evaluate(objective, X[b], **{k: (v[b:b + 1] if k == "per_problem" else v) for k, v in kw.items()})
            for b in range(X.shape[0])]


def _assert_inside(bad):
    assert not bad, "%d values outside their bound, first: %s" % (len(bad), bad[:3])


def _twin_policies(n):
    """(label, kwargs of oracle.evaluate) of every reduction the device kernels of n run: the exact butterfly and the fused
    one at every coordinates-per-lane count of the built mappings that cover n"""
    out = [("exact", dict(reduction="butterfly", width=_width(n)))]
    for E in (1, 2, 4):
        if 64 * E >= n:
            out.append(("fma", dict(reduction="butterfly_fma", width=max(_width(n), E), fma_group=E)))
    return out


def test_rosenbrock_and_diag_quadratic_twins_are_within_the_bounds(oracle):
    worst, bad = Cs.Worst(), []
    for n in Cs.DIMS:
        X = Cs.inputs(n)
        a, c = Cs.diag_coefficients(n)
        for name, refs, ks, kw in (("rosenbrock", Cs.rosenbrock_reference(n), hp.rosenbrock_k(n), {}),
                                   ("diag_quadratic", Cs.diag_quadratic_reference(n), hp.diag_quadratic_k(n),
                                    dict(params=np.concatenate([a, [c]])))):
            for label, policy in _twin_policies(n):
                for b, (f, g) in enumerate(_rows(oracle, name, X, **kw, **policy)):
                    bad += Cs.audit(refs[b], f, g, ks, worst=worst, label="%s %s " % (name, label),
                                    what="%s n=%d %s %s" % (name, n, label, Cs.FAMILIES[b]))
    REPORTS.report("mpmath bound, fp64 twins (error / bound)", worst)
    _assert_inside(bad)


def test_float_twins_are_within_the_bounds():
    import l32_lib
    worst, bad = Cs.Worst(), []
    for n in Cs.DIMS:
        X = Cs.inputs(n, "float32")
        a, c = Cs.diag_coefficients(n, "float32")
        for name, oid, refs, ks, params in (
                ("rosenbrock", l32_lib.ROSENBROCK, Cs.rosenbrock_reference(n, "float32"), hp.rosenbrock_k(n), None),
                ("diag_quadratic", l32_lib.DIAG_QUADRATIC, Cs.diag_quadratic_reference(n, "float32"),
                 hp.diag_quadratic_k(n), np.concatenate([a, [c]]))):
            f, g = l32_lib.twin_eval(oid, X, params, width=l32_lib.padded_width(n))
            assert f.dtype == np.float32 and g.dtype == np.float32
            for b in range(len(X)):
                bad += Cs.audit(refs[b], f[b], g[b], ks, dtype="float32", worst=worst, label=name + " ",
                                what="%s float32 n=%d %s" % (name, n, Cs.FAMILIES[b]))
    REPORTS.report("mpmath bound, float32 twin (error / bound)", worst)
    _assert_inside(bad)


def test_hessian_twins_are_within_the_bounds():
    """hess_full through the derivative checker's twin (entry [b, j, i] = H(i, j)); n <= 64, one coordinate per lane."""
    import dv_cases
    import dv_lib
    worst, bad = Cs.Worst(), []
    for n in [n for n in Cs.DIMS if n <= 64]:
        X = Cs.inputs(n)
        a, c = Cs.diag_coefficients(n)
        for name, oid, refs, ks, params in (
                ("rosenbrock", dv_lib.ROSENBROCK, Cs.rosenbrock_reference(n, hessian=True), hp.rosenbrock_k(n), None),
                ("diag_quadratic", dv_lib.DIAG_QUADRATIC, Cs.diag_quadratic_reference(n, hessian=True),
                 hp.diag_quadratic_k(n), np.concatenate([a, [c]]))):
            out = dv_lib.twin_check(oid, X, params, dv_cases.config(0), hessian=True)
            for b in range(len(X)):
                bad += Cs.audit(refs[b], out["f"][b], out["grad"][b], ks, H=out["hess"][b].T, worst=worst, label=name + " ",
                                what="%s derivatives n=%d %s" % (name, n, Cs.FAMILIES[b]))
    REPORTS.report("mpmath bound, derivative-check twin (error / bound)", worst)
    _assert_inside(bad)


def _gram_mapping(n):
    P = 8
    while P < n:
        P <<= 1
    return P, (1 if P == 8 else (4 if P == 256 else 2))


def test_ridge_twins_are_within_the_bounds(oracle):
    worst, bad = Cs.Worst(), []
    for rows, n in Cs.RIDGE_SHAPES + Cs.RIDGE_GRAM_SHAPES:
        A, Y, X = Cs.ridge_data(rows, n)
        R, refs = Cs.ridge_reference(rows, n)
        params = oracle.ridge_params(A, Cs.RIDGE_LAMBDA)
        P, E = _gram_mapping(n)
        forms = [("gram", "squared_error_ridge_gram", dict(reduction="butterfly_fma", width=P, fma_group=E))]
        if (rows, n) in Cs.RIDGE_SHAPES:
            forms += [("valu", "squared_error_ridge", dict(reduction="butterfly", width=_width(n))),
                      ("mfma", "squared_error_ridge_mfma", dict(reduction="butterfly", width=64))]
        for label, name, policy in forms:
            for b, (f, g) in enumerate(_rows(oracle, name, X, params=params, per_problem=Y, **policy)):
                bad += Cs.audit(refs[b], f, g, R.k(), worst=worst, label=label + " ",
                                what="ridge %s (%d, %d) %s" % (label, rows, n, Cs.FAMILIES[b]))
        As, Yo, Xo = Cs.ridge_own_data(rows, n)
        import cppnumericalsolvers_amd.engine as engine
        data = engine.ridge_per_problem_rows(As, Yo)
        own = _rows(oracle, "squared_error_ridge_own_gram", Xo, params=np.array([float(rows), Cs.RIDGE_LAMBDA]),
                    per_problem=data, reduction="butterfly_fma", width=P, fma_group=E)
        for b, (f, g) in enumerate(own):
            bad += Cs.audit(Cs.ridge_own_reference(rows, n)[b], f, g, (n + rows, n + rows), worst=worst, label="own ",
                            what="ridge own (%d, %d) %s" % (rows, n, Cs.FAMILIES[b]))
    REPORTS.report("mpmath bound, ridge twins (error / bound)", worst)
    _assert_inside(bad)


def al_problem(n, terms, n_eq):
    """the term table as tests/auglag_lib.py describes it to the oracle"""
    import auglag_lib as al
    mk = lambda t: al.term([(p[0],) if p[1] is None and p[2] == 0.0 else (p[0], p[1], p[2]) for p in t[0]], t[1], t[2],
                           product=t[3])
    return al.Problem(n, mk(terms[0]), [mk(t) for t in terms[1:1 + n_eq]], [mk(t) for t in terms[1 + n_eq:]])


@pytest.mark.parametrize("n", Cs.COMPOSITE_DIMS)
def test_composite_twin_is_within_the_bound(oracle, n):
    import auglag_lib as al
    worst, bad = Cs.Worst(), []
    for n_eq, n_ineq in ((0, 0), (1, 0), (0, 1), (2, 2), (4, 0), (0, 4), (3, 1), (4, 4)):
        terms, X, lam, mu, rho = Cs.composite_case(n, n_eq, n_ineq)
        k = hp.composite_k(n, terms)
        f, g = al.oracle_eval(al_problem(n, terms, n_eq), X, lam, mu, rho, reduction="butterfly", width=_width(n))
        for b, ev in enumerate(Cs.composite_reference(n, n_eq, n_ineq)):
            bad += Cs.audit(ev, f[b], g[b], (k, k), worst=worst, label="",
                            what="composite n=%d eq=%d ineq=%d %s" % (n, n_eq, n_ineq, Cs.FAMILIES[b]))
    REPORTS.report("mpmath bound, composite twin (error / bound)", worst)
    _assert_inside(bad)


# ---- 3. the bounds see a wrong kernel ---------------------------------------------------------------------------------------
def _floats(ev):
    """the definition rounded to double: what a correct kernel could return at best"""
    return float(ev.f), [float(v) for v in ev.g]


MUTANT_DIMS = (2, 3, 9, 33, 256)


def _seen(n, b, mutate, ks):
    """a wrong kernel (the correctly rounded definition with `mutate` applied in exact arithmetic) is outside the bound"""
    x = hp.vec(Cs.inputs(n)[b])
    ev = Cs.rosenbrock_reference(n)[b]
    f, g = mutate(x, ev.f, list(ev.g))
    return bool(Cs.audit(ev, float(f), [float(v) for v in g], ks))


def _mutant_cases(skip):
    return [(n, b) for n in MUTANT_DIMS for b in range(len(Cs.FAMILIES)) if not skip(n, Cs.FAMILIES[b])]


def test_correctly_rounded_definition_is_inside_every_bound():
    """the control of the mutants below: without a mutation nothing is flagged"""
    for n in MUTANT_DIMS:
        for b, ev in enumerate(Cs.rosenbrock_reference(n)):
            f, g = _floats(ev)
            assert not Cs.audit(ev, f, g, hp.rosenbrock_k(n))


def test_bound_sees_rosenbrock_without_its_last_term():
    # degenerate: in the minimiser's 1e-7 neighbourhood the dropped term is ~1e-12, at the level of u F_abs itself
    skip = lambda n, family: family == "near_minimiser"
    for n, b in _mutant_cases(skip):
        drop = lambda x, f, g: (f - hp.rosenbrock_term(hp._PLAIN, x[-2], x[-1]), g)
        assert _seen(n, b, drop, hp.rosenbrock_k(n)), (n, Cs.FAMILIES[b])


def test_bound_sees_a_padding_coordinate_treated_as_real():
    """x_n = 0 taken as a coordinate: the extra term (1 - x_{n-1})^2 + 100 x_{n-1}^4"""
    for n, b in _mutant_cases(lambda n, family: False):
        pad = lambda x, f, g: (f + hp.rosenbrock_term(hp._PLAIN, x[-1], mpf(0)), g)
        assert _seen(n, b, pad, hp.rosenbrock_k(n)), (n, Cs.FAMILIES[b])


def test_bound_sees_the_gradient_without_its_backward_half_at_the_last_coordinate():
    # degenerate: on the row that is zero but for x_0, t2_{n-2} = x_{n-1} - x_{n-2}^2 is exactly 0 once n > 2
    skip = lambda n, family: family == "one_hot_first" and n > 2
    for n, b in _mutant_cases(skip):
        def half(x, f, g):
            g[-1] -= hp.rosenbrock_gradient_backward(hp._PLAIN, x[-2], x[-1])
            return f, g
        assert _seen(n, b, half, hp.rosenbrock_k(n)), (n, Cs.FAMILIES[b])


def test_bound_sees_the_ridge_gradient_without_its_regulariser():
    for rows, n in Cs.RIDGE_SHAPES:
        R, refs = Cs.ridge_reference(rows, n)
        X = Cs.ridge_data(rows, n)[2]
        for b, ev in enumerate(refs):
            assert not Cs.audit(ev, *_floats(ev), R.k())
            if Cs.FAMILIES[b] == "tiny":   # degenerate: 2 lam x ~ 1e-161 beside a gradient of -2 A^T y ~ 1
                continue
            x = hp.vec(X[b])
            g = [float(ev.g[j] - 2 * R.lam * x[j]) for j in range(n)]
            assert Cs.audit(ev, float(ev.f), g, R.k()), (rows, n, Cs.FAMILIES[b])


# ---- 4. the result postconditions on the twins ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", Cs.RESULT_DIMS)
@pytest.mark.parametrize("name", ["rosenbrock", "diag_quadratic"])
def test_result_postconditions_hold_on_the_twins(oracle, name, n):
    """tests/test_gpu_results_mpmath.py's audit on the CPU twins of the Lbfgs family, from the same starts: every
    postcondition holds and NO problem ends on a non-finite bail-out."""
    params, evaluate, ks, minimiser, mu = Cs.result_objective(name, n)
    blob = None if params is None else np.concatenate([params[0], [params[1]]])
    x0 = Cs.result_starts(name, n)
    lower, upper = Cs.result_box(n)
    worst, bad = Cs.Worst(), []
    for stop_name, stop in (("default", oracle.default_stop()), ("parity", oracle.parity_stop())):
        runs = [("lbfgs exact", x0, {}, oracle.minimize_batch(name, x0, m=10, stop=stop, params=blob, reduction="butterfly",
                                                              width=_width(n))),
                ("lbfgs fma", x0, {}, oracle.minimize_batch(name, x0, m=10, stop=stop, params=blob,
                                                            reduction="butterfly_fma", width=_width(n), fma_group=1)),
                ("lbfgs hager_zhang", x0, {}, oracle.minimize_batch(name, x0, m=10, stop=stop, params=blob,
                                                                    reduction="butterfly", width=_width(n),
                                                                    linesearch="hager_zhang")),
                ("bfgs", x0, {}, oracle.bfgs_minimize_batch(name, x0, stop=stop, params=blob, reduction="butterfly",
                                                            width=_width(n)))]
        xb = np.clip(x0, lower, upper)
        lstop = oracle.lbfgsb_default_stop() if stop_name == "default" else stop
        runs.append(("lbfgsb", xb, dict(lower=lower, upper=upper, lbfgsb=True),
                     oracle.lbfgsb_minimize_batch(name, xb, m=5, stop=lstop, params=blob, lower=lower, upper=upper,
                                                  reduction="butterfly", width=_width(n))))
        for label, start, kw, (x, f, g, p) in runs:
            convex = {} if (minimiser is None or "lbfgsb" in label) else dict(minimiser=minimiser, mu=mu)
            b, excluded = Cs.audit_results(evaluate, ks, start, x, f, g, p, lstop if "lbfgsb" in label else stop,
                                           worst=worst, label=label + " ",
                                           what="%s n=%d %s %s" % (name, n, label, stop_name), **kw, **convex)
            assert excluded == 0, (label, stop_name)
            bad += b
    REPORTS.report("mpmath bound, returned f and g of the twins (error / bound)", worst)
    _assert_inside(bad)


def test_augmented_lagrangian_report_holds_on_the_twin(oracle):
    """every case of the GPU test, on the twin first"""
    import auglag_lib as al
    worst, bad = Cs.Worst(), []
    for n, n_eq, n_ineq in Cs.AL_REPORT_CASES:
        terms, x0 = Cs.al_report_case(n, n_eq, n_ineq)
        o = al.oracle_minimize(al_problem(n, terms, n_eq), x0, config=al.default_config(outer_num_iterations=30),
                               reduction="butterfly", width=_width(n))
        bad += Cs.audit_al_report(terms, n_eq, o["x"], o["lambda"], o["mu"], o["max_violation"],
                                  o["max_lagrangian_gradient"], worst=worst, what="n=%d" % n)
    REPORTS.report("mpmath bound, augmented-Lagrangian report of the twin (error / bound)", worst)
    _assert_inside(bad)


@pytest.mark.parametrize("rows,n", Cs.RIDGE_RESULT_SHAPES)
def test_result_postconditions_hold_on_the_ridge_twins(oracle, rows, n):
    """the four ridge forms from the starts of the GPU test: every postcondition, the minimiser inequality of all four
    (one 200-bit LU per matrix), no bail-out.  At 128 x 64 the first 4 problems of every batch are audited at 200 bits
    (the device test audits them all) and every problem is shown to end finite."""
    audited = slice(0, 4 if rows * n > 2000 else Cs.RESULT_B)
    import cppnumericalsolvers_amd.engine as engine
    A, Y, x0, evaluate, ks, minimiser, mu = Cs.ridge_result_case(rows, n)
    As, Yo, x0o, evaluate_own, ks_own, minimiser_own, mu_own = Cs.ridge_own_result_case(rows, n)
    params = oracle.ridge_params(A, Cs.RIDGE_LAMBDA)
    P, E = _gram_mapping(n)
    worst, bad = Cs.Worst(), []
    for stop_name, stop in (("default", oracle.default_stop()), ("parity", oracle.parity_stop())):
        for label, name, policy in (
                ("valu", "squared_error_ridge", dict(reduction="butterfly", width=_width(n))),
                ("mfma", "squared_error_ridge_mfma", dict(reduction="butterfly", width=64)),
                ("gram", "squared_error_ridge_gram", dict(reduction="butterfly_fma", width=P, fma_group=E))):
            x, f, g, p = oracle.minimize_batch(name, x0, m=10, stop=stop, params=params, per_problem=Y, **policy)
            assert np.isfinite(x).all() and np.isfinite(f).all() and np.isfinite(g).all(), (label, stop_name)
            b, excluded = Cs.audit_results(evaluate, ks, x0[audited], x[audited], f[audited], g[audited], p[audited], stop,
                                           minimiser=minimiser, mu=mu, worst=worst, label=label + " ",
                                           what="ridge %s (%d, %d) %s" % (label, rows, n, stop_name))
            assert excluded == 0, (label, stop_name)
            bad += b
        x, f, g, p = oracle.minimize_batch("squared_error_ridge_own_gram", x0o, m=10, stop=stop,
                                           params=np.array([float(rows), Cs.RIDGE_LAMBDA]),
                                           per_problem=engine.ridge_per_problem_rows(As, Yo), reduction="butterfly_fma",
                                           width=P, fma_group=E)
        assert np.isfinite(x).all() and np.isfinite(f).all() and np.isfinite(g).all(), ("own", stop_name)
        b, excluded = Cs.audit_results(evaluate_own, ks_own, x0o[audited], x[audited], f[audited], g[audited], p[audited],
                                       stop, minimiser=minimiser_own, mu=mu_own, worst=worst, label="own ",
                                       what="ridge own (%d, %d) %s" % (rows, n, stop_name))
        assert excluded == 0, ("own", stop_name)
        bad += b
    REPORTS.report("mpmath bound, returned f and g of the ridge twins (error / bound)", worst)
    _assert_inside(bad)


@pytest.mark.parametrize("n", Cs.RESULT_DIMS)
def test_result_postconditions_hold_on_the_composite_twin(oracle, n):
    """Lbfgs on the composite from the starts of the GPU test: every postcondition, no bail-out"""
    import auglag_lib as al
    terms, n_eq, x0, lam, mu, rho, evaluate, k = Cs.composite_result_case(n)
    worst, bad = Cs.Worst(), []
    for stop_name, stop in (("default", oracle.default_stop()), ("parity", oracle.parity_stop())):
        x, f, g, p = al.oracle_composite_minimize(al_problem(n, terms, n_eq), x0, lam, mu, rho, stop=stop,
                                                  reduction="butterfly", width=_width(n))
        b, excluded = Cs.audit_results(evaluate, (k, k), x0, x, f, g, p, stop, worst=worst, label="composite ",
                                       what="composite n=%d %s" % (n, stop_name))
        assert excluded == 0, stop_name
        bad += b
    REPORTS.report("mpmath bound, returned f and g of the composite twin (error / bound)", worst)
    _assert_inside(bad)


_PARITY = dict(x_delta=1e-11, gradient_norm=1e-8, past=0)


def _record_stop(lib, **over):
    """(the stopping record a twin library takes, the same fields as attributes for the audit)"""
    import types
    fields = {**lib.STOP_PRESETS["default"], **over}
    return lib.make_stop(**fields), types.SimpleNamespace(**fields)


@pytest.mark.parametrize("n", Cs.RESULT_DIMS)
@pytest.mark.parametrize("name", ["rosenbrock", "diag_quadratic"])
def test_result_postconditions_hold_on_the_twins_of_the_other_solvers(name, n):
    """The float L-BFGS, TrustRegionNewton, NewtonDescent, GradientDescent, ConjugatedGradientDescent and NelderMead
    (value only) twins in device order, from the same starts: every postcondition, no bail-out."""
    import fo_lib
    import l32_lib
    import nd_lib
    import nm_lib
    import tr_lib
    oid = 0 if name == "rosenbrock" else 1
    # the conjugate-gradient twin runs Rosenbrock to the iteration limit, a second per row from n = 33 on: there it takes
    # the first 8 starts (one per host thread); the device test audits all 24
    cg_rows = 8 if (name == "rosenbrock" and n >= 33) else Cs.RESULT_B
    worst, bad = Cs.Worst(), []
    for stop_name, over in (("default", {}), ("parity", _PARITY)):
        runs = []
        for dtype, solve in (("float32", None), ("float64", None)):
            params, evaluate, ks, minimiser, mu = Cs.result_objective(name, n, dtype)
            blob = None if params is None else np.concatenate([params[0], [params[1]]])
            x0 = Cs.result_starts(name, n).astype(np.float32 if dtype == "float32" else np.float64)
            convex = {} if minimiser is None else dict(minimiser=minimiser, mu=mu)
            if dtype == "float32":
                rec, stop = _record_stop(l32_lib, **over)
                runs.append(("lbfgs float32", dtype, x0, evaluate, ks, stop, convex, {},
                             l32_lib.twin_solve(oid, 6, x0, blob, rec, order=l32_lib.DEVICE_ORDER)))
                continue
            for label, lib, call in (
                    ("trust_region", tr_lib, lambda r: tr_lib.twin_solve(oid, x0, blob, r, order=tr_lib.DEVICE_ORDER)),
                    ("newton_descent", nd_lib, lambda r: nd_lib.twin_solve(oid, x0, blob, r, order=nd_lib.DEVICE_ORDER)),
                    # (rows over eight host threads: the Armijo search of the conjugated-gradient twin runs the full
                    #  10 000 iterations on Rosenbrock)
                    ("gradient_descent", fo_lib,
                     lambda r: fo_lib.twin_solve_threaded(fo_lib.GRADIENT_DESCENT, oid, x0, blob, r,
                                                          order=fo_lib.DEVICE_ORDER)),
                    ("conjugated_gradient_descent", fo_lib,
                     lambda r: fo_lib.twin_solve_threaded(fo_lib.CONJUGATED_GRADIENT_DESCENT, oid, x0[:cg_rows], blob, r,
                                                          order=fo_lib.DEVICE_ORDER))):
                rec, stop = _record_stop(lib, **over)
                start = x0[:cg_rows] if label == "conjugated_gradient_descent" else x0
                runs.append((label, dtype, start, evaluate, ks, stop, convex, {}, call(rec)))
            rec, stop = _record_stop(nm_lib, **over)
            runs.append(("nelder_mead", dtype, x0, evaluate, ks, stop, {}, dict(value_only=True),
                         nm_lib.twin_solve(oid, x0, blob, rec, order=nm_lib.DEVICE_ORDER)[:4]))
        for label, dtype, x0, evaluate, ks, stop, convex, kw, (x, f, g, p) in runs:
            b, excluded = Cs.audit_results(evaluate, ks, x0, x, f, g, p, stop, dtype=dtype, worst=worst, label=label + " ",
                                           what="%s n=%d %s %s" % (name, n, label, stop_name), **kw, **convex)
            assert excluded == 0, (label, stop_name)
            bad += b
    REPORTS.report("mpmath bound, returned f and g of the other twins (error / bound)", worst)
    _assert_inside(bad)


@pytest.mark.parametrize("n", Cs.COMPOSITE_DIMS)
def test_bound_sees_a_wrong_composite(n):
    """The composite's k is a sum over its terms and therefore loose; it still sees a composite without one of its
    constraints, and one that takes the wrong branch of a max(0, .): the clamped branch where the inequality is active,
    the open branch where it is not.  (Row 0, which sits on the kink, is the degenerate case of the second mutant: the two
    branches agree there.)"""
    n_eq, n_ineq = 2, 2
    terms, X, lam, mu, rho = Cs.composite_case(n, n_eq, n_ineq)
    k = hp.composite_k(n, terms)
    refs = Cs.composite_reference(n, n_eq, n_ineq)
    for b, ev in enumerate(refs):
        assert not Cs.audit(ev, *_floats(ev), (k, k))
        for dropped in range(1, len(terms)):          # every constraint in turn
            kept = [t for i, t in enumerate(terms) if i != dropped]
            eq = n_eq - (dropped <= n_eq)
            wrong = hp.composite(X[b], kept, eq, np.delete(lam[b], dropped - 1) if dropped <= n_eq else lam[b],
                                 np.delete(mu[b], dropped - 1 - n_eq) if dropped > n_eq else mu[b], rho[b])
            if dropped > n_eq and Cs.FAMILIES[b] == "large":
                # degenerate: on the 1e3 row this inequality is inactive and contributes the constant -mu^2 / (2 rho) ~ 1
                # alone, less than one unit in the last place of a value of 1e16
                v = hp._term(hp._PLAIN, hp._mpf_term(hp._PLAIN, terms[dropped]), hp.vec(X[b]))[0]
                if mpf(float(mu[b][dropped - 1 - n_eq])) - mpf(float(rho[b])) * v <= 0:
                    continue
            assert Cs.audit(ev, *_floats(wrong), (k, k)), (n, Cs.FAMILIES[b], "dropped term", dropped)
        if b == 0:
            continue
        x = hp.vec(X[b])
        plain = [hp._mpf_term(hp._PLAIN, t) for t in terms]
        for q in range(n_ineq):                        # the other branch of inequality q
            v, gv = hp._term(hp._PLAIN, plain[1 + n_eq + q], x)
            m, r = mpf(float(mu[b][q])), mpf(float(rho[b]))
            t = m - r * v
            # active (t > 0): clamped instead, the part (t^2 - mu^2) / (2 rho) becomes -mu^2 / (2 rho), its gradient 0;
            # inactive: opened instead, the same change with the other sign
            sign = -1 if t > 0 else 1
            f = ev.f + sign * t * t / (2 * r)
            g = [ev.g[j] - sign * t * gv[j] for j in range(n)]
            assert Cs.audit(ev, float(f), [float(e) for e in g], (k, k)), (n, Cs.FAMILIES[b], "wrong branch", q)

