"""tests/step_lib.py on the CPU: the replay checks itself, every CPU twin trajectory of tests/step_cases.py passes every check
inside both caps (the reference-order twin, which tests/test_reference_programs.py and tests/test_oracle.py hold to the
compiled reference bit for bit, among them: the reference measured against the bounds), and a trajectory generator that
carries a planted bug lands outside.

One line per family goes to the terminal summary (conftest._SUMMARY_LINES) and into DESIGN.md section 5.
"""
import numpy as np
import pytest

import hp_lib as hp
import step_cases as Sc
import step_lib as St

mp, mpf = hp.mp, hp.mpf
TOL = mpf(10) ** -40
LINES = []


@pytest.fixture(scope="module", autouse=True)
def _lines_to_the_terminal_summary():
    yield
    import conftest
    conftest._SUMMARY_LINES.extend(LINES)


# ---- 1. the replay checks itself -------------------------------------------------------------------------------------------
def _quadratic(n, seed):
    """a strictly convex quadratic 0.5 x^T A x - b^T x at 200 bits"""
    rng = np.random.default_rng(seed)
    Q = rng.normal(size=(n, n))
    A = [hp.vec(r) for r in (Q.T @ Q + np.eye(n))]
    A = [[(A[i][j] + A[j][i]) / 2 for j in range(n)] for i in range(n)]
    return A, hp.vec(rng.normal(size=n)), hp.vec(rng.normal(size=n))


def _exact_line_steps(A, b, x, steps, h0, dense):
    """BFGS with exact line steps from x: the pairs and the directions H_k g_k"""
    n = len(x)
    pairs, directions = [], []
    g = [mp.fdot(A[i], x) - b[i] for i in range(n)]
    for _ in range(steps):
        d = St.direction(pairs, h0, g, dense=dense)
        directions.append((d, g, x))
        Ad = St.matvec(A, d)
        alpha = mp.fdot(g, d) / mp.fdot(d, Ad)
        xn = [x[j] - alpha * d[j] for j in range(n)]
        gn = [mp.fdot(A[i], xn) - b[i] for i in range(n)]
        s, y = [xn[j] - x[j] for j in range(n)], [gn[j] - g[j] for j in range(n)]
        pairs.append((s, y, mp.fdot(s, y)))
        x, g = xn, gn
    return pairs, directions


@pytest.mark.parametrize("dense", [True, False])
def test_nth_direction_on_a_quadratic_is_the_newton_direction(dense):
    """exact line steps, m >= n: the n-th direction H_{n-1} g_{n-1} with its exact line step is the Newton step A^-1 g_{n-1}
    (the directions are conjugate: the n-th step ends on the minimiser), and with the n-th pair H_n is A^-1 itself"""
    for n in (2, 5, 9):
        A, b, x0 = _quadratic(n, n)
        pairs, directions = _exact_line_steps(A, b, x0, n, [mpf(1)] * n, dense)
        d, g, x = directions[-1]
        alpha = mp.fdot(g, d) / mp.fdot(d, St.matvec(A, d))
        newton = mp.lu_solve(mp.matrix(A), mp.matrix(g))
        scale = max(abs(v) for v in newton)
        assert all(abs(alpha * d[j] - newton[j]) <= TOL * scale for j in range(n)), n
        v = hp.vec(np.random.default_rng(n).normal(size=n))
        Hv, Av = St.direction(pairs, [mpf(1)] * n, v, dense=dense), mp.lu_solve(mp.matrix(A), mp.matrix(v))
        assert all(abs(Hv[j] - Av[j]) <= TOL * max(abs(e) for e in Av) for j in range(n)), n


def test_matrix_update_satisfies_the_secant_equation():
    """H_k y_{k-1} = s_{k-1} after every update, from gamma I and from a diagonal H_0"""
    n = 6
    A, b, x0 = _quadratic(n, 21)
    for h0 in ([mpf(3) / 7] * n, hp.vec(np.linspace(0.2, 5.0, n))):
        pairs, _ = _exact_line_steps(A, b, x0, 4, h0, True)
        for k in range(1, len(pairs) + 1):
            s, y, _ = pairs[k - 1]
            Hy = St.matvec(St.dense_H(pairs[:k], h0), y)
            assert all(abs(Hy[j] - s[j]) <= TOL * max(abs(v) for v in s) for j in range(n)), k


def test_compact_representation_is_the_dense_matrix():
    """the form used above DENSE_MAX applies the same matrix as the dense update: 1e-40, scalar and diagonal H_0, on pairs
    that are not conjugate (random, with s^T y > 0)"""
    rng = np.random.default_rng(8)
    for n, p in ((3, 1), (7, 3), (9, 6)):
        pairs = []
        while len(pairs) < p:
            s, y = hp.vec(rng.normal(size=n)), hp.vec(rng.normal(size=n))
            if mp.fdot(s, y) > 0:
                pairs.append((s, y, mp.fdot(s, y)))
        g = hp.vec(rng.normal(size=n))
        for h0 in ([mpf(2) / 3] * n, hp.vec(rng.uniform(0.1, 4.0, n))):
            dense, compact = St.direction(pairs, h0, g, dense=True), St.direction(pairs, h0, g, dense=False)
            assert all(abs(a - c) <= TOL * max(abs(v) for v in dense) for a, c in zip(dense, compact)), (n, p)


def test_magnitude_companion_bounds_the_direction():
    """|H g| <= M entry by entry, and M' >= M"""
    rng = np.random.default_rng(9)
    n = 7
    pairs = []
    while len(pairs) < 4:
        s, y = hp.vec(rng.normal(size=n)), hp.vec(rng.normal(size=n))
        if mp.fdot(s, y) > 0:
            pairs.append((s, y, mp.fdot(s, y)))
    g, h0 = hp.vec(rng.normal(size=n)), [mpf(1) / 3] * n
    d, M = St.direction(pairs, h0, g), St.magnitude(pairs, h0, g)
    M1 = St.magnitude(pairs, h0, g, [mpf(10) ** -10] * 4, mpf(10) ** -10)
    assert all(abs(d[j]) <= M[j] <= M1[j] for j in range(n))


# ---- 2. the generator without a bug passes; with a planted bug it does not -------------------------------------------------------
def _numpy_objective(name, n, t):
    """(fun(x) -> (f, g) in t, hess_diag(x) or None) with a pairwise tree for the value"""
    one = lambda v: t(v)
    if name.startswith("rosenbrock"):
        def fun(x):
            t1, t2 = one(1) - x[:-1], x[1:] - x[:-1] * x[:-1]
            g = np.zeros(n, dtype=t)
            g[:-1] += one(-2) * t1 - one(400) * x[:-1] * t2
            g[1:] += one(200) * t2
            return St.tree_dot(np.ones(n - 1, dtype=t), t1 * t1 + one(100) * t2 * t2), g

        def hess_diag(x):
            h = np.zeros(n, dtype=t)
            h[:-1] += one(1200) * x[:-1] * x[:-1] - one(400) * x[1:] + one(2)
            h[1:] += one(200)
            return h
    else:
        a, c = Sc.diag_coefficients(n, "float32" if t is np.float32 else "float64")
        a = a.astype(t)

        def fun(x):
            return St.tree_dot(a * x, x) + one(c), one(2) * a * x

        def hess_diag(x):
            return one(2) * a
    return fun, (hess_diag if name.endswith("_second") else None)


GENERATOR_SHAPES = (("rosenbrock", "std", 2, 1), ("rosenbrock", "u2", 8, 6), ("rosenbrock", "std", 17, 3),
                    ("diag_quadratic", "std", 7, 3), ("diag_quadratic", "u2", 33, 6), ("rosenbrock_second", "std", 8, 3),
                    ("diag_quadratic_second", "std", 7, 3))
# float32: with six pairs the counted slack of g^T d (K u |g|^T M') passes g^T d itself on Rosenbrock and the reset
# decision is undecidable from iteration 12 on, and with three from the `std` starts: the float rows keep to what stays decidable
GENERATOR_SHAPES_F32 = (("rosenbrock", "std", 2, 1), ("rosenbrock", "std", 9, 1), ("rosenbrock", "u2", 17, 3),
                        ("rosenbrock", "u2", 33, 3), ("diag_quadratic", "std", 7, 6), ("diag_quadratic", "u2", 33, 3))


def _generated(name, start, n, m, bug=None, dtype="float64"):
    t = np.float32 if dtype == "float32" else np.float64
    fun, hd = _numpy_objective(name, n, t)
    x0 = Sc.starts(start, n, dtype)[list(Sc.TRACED[:4])]
    return [St.generate(fun, x0[b], m, Sc.limit(m), Sc.GRADIENT_NORM, t, bug=bug, hess_diag=hd) for b in range(len(x0))]


def _audit_generated(name, start, n, m, bug=None, dtype="float64"):
    rules = St.Rules(m, dtype=dtype, second=name.endswith("_second"))
    return St.audit_case(_generated(name, start, n, m, bug, dtype), rules, hess_diag=Sc.hess_diag(name, n),
                         what="%s %s n=%d m=%d" % (name, start, n, m))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_generator_without_a_bug_is_inside_the_bounds_and_the_caps(dtype):
    total = St.Report()
    for name, start, n, m in (GENERATOR_SHAPES if dtype == "float64" else GENERATOR_SHAPES_F32):
        rep = _audit_generated(name, start, n, m, dtype=dtype)
        Sc.assert_case(rep, m, "generator %s %s n=%d m=%d %s" % (name, start, n, m, dtype))
        total.merge(rep)
    assert total.evictions > 0 and total.audited > 100
    LINES.append("step audit, generator %s: %s" % (dtype, total.line()))


_CLEAN = {}


def _clean(name, start, n, m):
    """the report of the generator without a bug (kept: every planted bug asks for it)"""
    key = (name, start, n, m)
    if key not in _CLEAN:
        _CLEAN[key] = _audit_generated(name, start, n, m)
    return _CLEAN[key]


def _touches(bug, name, start, n, m):
    """The cases a planted bug can show on.  The search that accepts on sufficient decrease alone is listed for First-mode
    Rosenbrock only: on the convex quadratics, and on Rosenbrock under its diagonal preconditioner, the unit step of the
    quasi-Newton direction meets both conditions, the buggy search ends where the right one does on all but 2 of 144 (1 of
    72) iterations, and the case stays under the cap on exceptions."""
    clean = _clean(name, start, n, m)
    longest = max(total for _, total in clean.audited_through)
    if bug == St.SECOND_AS_GAMMA:
        return name.endswith("_second")
    if bug in (St.EVICT_NEWEST, St.RING_ONE_OFF):
        return m >= 2 and clean.evictions > 0           # with one column the newest is the oldest
    if bug == St.SECOND_LOOP_REVERSED:
        return m >= 2 and longest >= 4                  # two pairs in the recursion; with one the reversed index is the index
    if bug == St.GAMMA_OLDEST:
        return m >= 2 and longest >= 4 and not name.endswith("_second")      # Second mode does not read gamma
    if bug == St.DECREASE_ALONE:
        return name == "rosenbrock"
    return True


@pytest.mark.parametrize("bug", St.BUGS)
def test_a_planted_bug_lands_outside(bug):
    """Outside = a direction past its bound, or a case past the cap on line-search exceptions.  The seventh bug of the list,
    a stored pair with s^T y <= 0, has no case: both searches end on the curvature condition, under which
    s^T y >= (1 - 0.9) |g^T s| > 0, and no input of tests/step_cases.py produces such a pair (0 pairs rejected on every
    row, generator and twins)."""
    seen = 0
    for name, start, n, m in GENERATOR_SHAPES:
        if not _touches(bug, name, start, n, m):
            continue
        rep = _audit_generated(name, start, n, m, bug=bug)
        outside = bool(rep.bad) or bool(St.caps(rep, m))
        assert outside, "%s: not seen on %s %s n=%d m=%d (%s)" % (bug, name, start, n, m, rep.line())
        seen += 1
    assert seen >= 2 or (bug == St.SECOND_AS_GAMMA and seen >= 1), bug


# ---- 3. every CPU twin trajectory passes every check, inside both caps --------------------------------------------------------
_ORACLE_NAME = {"rosenbrock": "rosenbrock", "rosenbrock_second": "rosenbrock", "diag_quadratic": "diag_quadratic"}


def _policy(family, n, E=1):
    if family == "reference":
        return dict(reduction="sequential")
    if family == "fma":
        return dict(reduction="butterfly_fma", width=max(Sc.width(n), E), fma_group=E)
    return dict(reduction="strided", width=256) if n > 256 else dict(reduction="butterfly", width=Sc.width(n))


def _rows(oracle, oname, X, blob, policy):
    if policy.get("reduction") == "strided":       # (oracle.evaluate has the two tree orders; the gradients have no sum in them)
        policy = dict(reduction="butterfly", width=Sc.width(X.shape[1]))
    out = [oracle.evaluate(oname, X[b], params=blob, **policy) for b in range(X.shape[0])]
    return np.array([f for f, _ in out]), np.array([g for _, g in out])


def _lbfgs_twin_report(oracle, family, name, start, n, m, E=1, linesearch="more_thuente"):
    blob, evaluate, ks = Sc.objective(name, n, sequential=(family == "reference"))
    policy = _policy(family, n, E)
    x0 = Sc.starts(start, n)[list(Sc.TRACED)]
    second = "functor" if name.endswith("_second") else False
    solve = lambda rows, fields: oracle.minimize_batch(_ORACLE_NAME[name], rows, m=m, stop=oracle.make_stop(**fields),
                                                       params=blob, second_mode=second, linesearch=linesearch, **policy)
    f0, g0 = _rows(oracle, _ORACLE_NAME[name], x0, blob, policy)
    rules = Sc.rules_of(family, m, linesearch=linesearch, second=bool(second))
    return St.audit_case(Sc.prefix_trajectories(solve, x0, f0, g0, m), rules, evaluate, ks, Sc.hess_diag(name, n),
                         what="%s %s %s n=%d m=%d" % (family, name, start, n, m))


def _finish(title, reports):
    total = St.Report()
    for m, what, rep in reports:
        Sc.assert_case(rep, m, what)
        total.merge(rep)
    LINES.append("step audit, %s: %s" % (title, total.line()))
    return total


@pytest.mark.parametrize("family,name,start,n,m", Sc.lbfgs_rows(("reference", "exact", "fma")))
def test_lbfgs_twins_are_inside_the_bounds_and_the_caps(oracle, family, name, start, n, m):
    """reference: the reference's own order (the compiled reference bit for bit); exact, fma: the kernels' twins, the fused
    one at the coordinates per lane of the library's mapping of n"""
    E = 1 if n <= 64 else (2 if n <= 128 else 4)
    rep = _lbfgs_twin_report(oracle, family, name, start, n, m, E=E)
    _finish("twin %s n=%d" % (family, n), [(m, "%s %s %s n=%d m=%d" % (family, name, start, n, m), rep)])


@pytest.mark.parametrize("name,start,n,m", Sc.MAPPING_SHAPES)
def test_fused_twins_of_every_lane_width_are_inside(oracle, name, start, n, m):
    """two and four coordinates per lane: the fused chain is another order of the same sums"""
    reports = []
    for E in sorted({E for _, E in Sc.mappings_of(n)} - {1 if n <= 64 else (2 if n <= 128 else 4)}):
        reports.append((m, "fma E=%d %s n=%d m=%d" % (E, name, n, m), _lbfgs_twin_report(oracle, "fma", name, start, n, m, E=E)))
    _finish("twin fma, other lane widths, n=%d" % n, reports)


@pytest.mark.parametrize("family,name,start,n,m", [(f,) + r for r in Sc.HZ_SHAPES for f in ("exact", "fma")]
                         + [("fma",) + Sc.LEAN_SHAPE])
def test_hager_zhang_and_lean_shape_twins_are_inside(oracle, family, name, start, n, m):
    """(the lean kernels are fused, four coordinates per lane)"""
    ls = "more_thuente" if (name, start, n, m) == Sc.LEAN_SHAPE else "hager_zhang"
    E = 4 if ls == "more_thuente" else 1
    rep = _lbfgs_twin_report(oracle, family, name, start, n, m, E=E, linesearch=ls)
    _finish("twin %s %s n=%d" % (family, ls, n), [(m, "%s %s %s n=%d m=%d" % (family, ls, name, n, m), rep)])


@pytest.mark.parametrize("name,start,n,m", Sc.F32_SHAPES)
def test_float32_twin_is_inside(name, start, n, m):
    import l32_lib
    blob, evaluate, ks = Sc.objective(name, n, "float32")
    oid = l32_lib.ROSENBROCK if name == "rosenbrock" else l32_lib.DIAG_QUADRATIC
    x0 = Sc.starts(start, n, "float32")[list(Sc.TRACED)]
    solve = lambda rows, fields: l32_lib.twin_solve(oid, m, rows, blob, l32_lib.make_stop(**fields),
                                                    order=l32_lib.DEVICE_ORDER)
    f0, g0 = l32_lib.twin_eval(oid, x0, blob, order=l32_lib.DEVICE_ORDER)
    rep = St.audit_case(Sc.prefix_trajectories(solve, x0, f0, g0, m), Sc.rules_of("f32", m, dtype="float32"), evaluate, ks,
                        what="float32 %s %s n=%d m=%d" % (name, start, n, m))
    _finish("twin float32 n=%d" % n, [(m, "float32 %s %s n=%d m=%d" % (name, start, n, m), rep)])


@pytest.mark.parametrize("name,start,n", Sc.BFGS_SHAPES)
def test_bfgs_twin_is_inside(oracle, name, start, n):
    m = Sc.BFGS_M
    blob, evaluate, ks = Sc.objective(name, n)
    policy = _policy("exact", n)
    x0 = Sc.starts(start, n)[list(Sc.TRACED)]
    solve = lambda rows, fields: oracle.bfgs_minimize_batch(name, rows, stop=oracle.make_stop(**fields), params=blob, **policy)
    f0, g0 = _rows(oracle, name, x0, blob, policy)
    rep = St.audit_case(Sc.prefix_trajectories(solve, x0, f0, g0, m), Sc.rules_of("bfgs", m, solver="bfgs"), evaluate, ks,
                        what="bfgs %s %s n=%d" % (name, start, n))
    _finish("twin bfgs n=%d" % n, [(m, "bfgs %s %s n=%d" % (name, start, n), rep)])


@pytest.mark.parametrize("relaxed", [False, True])
@pytest.mark.parametrize("per_problem", [False, True])
@pytest.mark.parametrize("name,start,n,m", Sc.LBFGSB_SHAPES)
def test_lbfgsb_twins_keep_the_box_and_the_decrease(oracle, name, start, n, m, per_problem, relaxed):
    blob, evaluate, ks = Sc.objective(name, n)
    lower, upper = Sc.box(n, per_problem)
    x0 = Sc.box_starts(start, n, lower, upper)
    call = oracle.lbfgsb_fast_minimize_batch if relaxed else oracle.lbfgsb_minimize_batch
    extra = {} if relaxed else _policy("exact", n)
    reports = []
    for b in Sc.TRACED:
        lo, hi = (lower[b], upper[b]) if per_problem else (lower, upper)
        solve = lambda rows, fields: call(name, rows, m=m, stop=oracle.make_stop(**fields), params=blob, lower=lo, upper=hi,
                                          **extra)
        f0, g0 = _rows(oracle, name, x0[b:b + 1], blob, _policy("exact", n))
        rules = Sc.rules_of("lbfgsb", m, solver="lbfgsb", lower=lo, upper=hi)
        reports.append(St.audit_case(Sc.prefix_trajectories(solve, x0[b:b + 1], f0, g0, m), rules, evaluate, ks,
                                     what="lbfgsb %s n=%d problem %d" % (name, n, b)))
    total = St.Report()
    for rep in reports:
        total.merge(rep)
    label = "lbfgsb %s %s n=%d" % ("relaxed" if relaxed else "exact", "own boxes" if per_problem else "shared box", n)
    _finish("twin " + label, [(m, label, total)])
