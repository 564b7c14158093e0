"""tests/bstep_lib.py on the CPU: the replay checks itself (the two solve routes and the two forms of B to 1e-40, the Cauchy
point as a minimiser of the model along the path), every CPU twin trajectory of tests/bstep_cases.py is inside the bound and
both caps, the branch counts (a)-(e) are positive on the reference-order twin with (a) on at least a tenth of the audited
iterations, and a generator written from the paper lands outside with each planted bug on every case the bug touches.

One line per family goes to the terminal summary (conftest._SUMMARY_LINES) and into DESIGN.md section 5.
"""
import numpy as np
import pytest

import bstep_cases as Bc
import bstep_lib as Bs
import hp_lib as hp
import step_lib as St

mp, mpf = hp.mp, hp.mpf
TOL = mpf(10) ** -40
LINES = []


@pytest.fixture(scope="module", autouse=True)
def _lines_to_the_terminal_summary():
    yield
    import conftest
    conftest._SUMMARY_LINES.extend(LINES)


# ---- 1. the replay checks itself ---------------------------------------------------------------------------------------------
def _pairs(n, p, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < p:
        s, y = hp.vec(rng.normal(size=n)), hp.vec(rng.normal(size=n))
        if mp.fdot(s, y) > 0:
            out.append((s, y))
    return out, mp.fdot(out[-1][1], out[-1][1]) / mp.fdot(out[-1][0], out[-1][1])


@pytest.mark.parametrize("n,p", [(3, 1), (7, 3), (9, 5), (17, 8)])
def test_the_two_forms_of_B_and_the_two_solve_routes_agree(n, p):
    """the matrix and the unrolled products are one operator, it satisfies every secant equation of the newest pair, it is
    theta I - W MM^-1 W^T (the compact form the sensitivity is taken from), and on a random free set the dense solve and the
    Woodbury route give one du: 1e-40"""
    pairs, theta = _pairs(n, p, 10 * n + p)
    dense, unrolled = Bs.Model(pairs, theta, n, dense=True), Bs.Model(pairs, theta, n, dense=False)
    rng = np.random.default_rng(n)
    v = hp.vec(rng.normal(size=n))
    a, b = dense.apply(v), unrolled.apply(v)
    scale = max(abs(e) for e in a)
    assert all(abs(a[j] - b[j]) <= TOL * scale for j in range(n))
    s, y = pairs[-1]
    Bs_ = dense.apply(s)
    assert all(abs(Bs_[j] - y[j]) <= TOL * max(abs(e) for e in y) for j in range(n))
    cf = Bs.Compact(pairs, theta, n, 0, mpf(0))
    mwv = cf.M(cf.wt(v))
    compact = [theta * v[j] - mp.fdot(cf.W[j], mwv) for j in range(n)]
    assert all(abs(a[j] - compact[j]) <= TOL * scale for j in range(n))
    free = sorted(rng.choice(n, size=max(1, n // 2), replace=False).tolist())
    r = hp.vec(rng.normal(size=len(free)))
    H = mp.matrix([[dense.matrix[i][j] for j in free] for i in free])
    du_dense = list(mp.lu_solve(H, mp.matrix([-e for e in r])))
    du_woodbury = Bs.woodbury(pairs, theta, free, r)
    top = max(abs(e) for e in du_dense)
    assert all(abs(c - d) <= TOL * top for c, d in zip(du_dense, du_woodbury))
    assert Bs.subspace_residual(unrolled, free, r, du_woodbury) <= TOL


@pytest.mark.parametrize("dense", [True, False])
def test_cauchy_point_is_the_first_minimiser_along_the_projected_path(dense):
    """by brute force: the model along P(x - t g) has a non-positive right derivative at every t before the Cauchy t and a
    non-negative one at it; the subspace step is stationary on the free set; both routes give one step"""
    n, p = 9, 3
    pairs, theta = _pairs(n, p, 77)
    rng = np.random.default_rng(5)
    rules = Bs.Rules(p, solver="lbfgsb")
    for trial in range(6):
        x, g = hp.vec(rng.uniform(0.2, 0.8, n)), hp.vec(rng.normal(size=n) * 3.0 ** trial)
        lo, hi = [mpf(0)] * n, [mpf(1)] * n
        st = Bs.replay_step(x, g, lo, hi, pairs, theta, rules, dense=dense, bounds=False)
        B = Bs.Model(pairs, theta, n)

        def path(t):
            return [min(max(x[j] - t * g[j], lo[j]), hi[j]) - x[j] for j in range(n)]

        def model(z):
            return mp.fdot(g, z) + mp.fdot(z, B.apply(z)) / 2

        h = mpf(10) ** -30
        ts = [st.t * k / 40 for k in range(40)]
        assert all(model(path(t + h)) <= model(path(t)) for t in ts), trial
        if st.t > 0 or st.crossed:
            assert model(path(st.t + h)) >= model(path(st.t)) - mpf(10) ** -50, trial
        zc = path(st.t)
        assert all(abs(zc[j] - st.z[j]) <= TOL for j in range(n)), trial
        if st.free:
            grad = B.apply([st.z[j] + (st.du[st.free.index(j)] if j in st.free else 0) for j in range(n)])
            assert all(abs(g[j] + grad[j]) <= TOL * max(abs(e) for e in g) for j in st.free), trial
            assert all(lo[j] - TOL <= x[j] + st.d[j] <= hi[j] + TOL for j in range(n)), trial


# ---- 2. the generator without a bug passes; with a planted bug it does not ---------------------------------------------------------
def _numpy_objective(name, n):
    if name == "rosenbrock":
        def fun(x):
            t1, t2 = 1.0 - x[:-1], x[1:] - x[:-1] * x[:-1]
            g = np.zeros(n)
            g[:-1] += -2.0 * t1 - 400.0 * x[:-1] * t2
            g[1:] += 200.0 * t2
            return St.tree_dot(np.ones(n - 1), t1 * t1 + 100.0 * t2 * t2), g
    else:
        a, c = Bc.coefficients(n)

        def fun(x):
            return St.tree_dot(a * x, x) + c, 2.0 * a * x
    return fun


_GENERATED = {}
U = float(hp.U["float64"])


def _shows(change, x, xn, lo, hi, st):
    """whether a planted bug changed, by more than twice the bound (once for the double d with the bug, once for the one
    without), the part of d that the next iterate shows: the coordinates not on a bound there, up to the scale that the
    search is free to choose (with no free variable: every coordinate, at the scale 1)"""
    with_bug, without = change
    inside = [j for j in range(len(x)) if xn[j] != lo[j] and xn[j] != hi[j]] if st.free else list(range(len(x)))
    if not inside:
        return False
    a, b = with_bug[inside], without[inside]
    c = float(a @ b) / float(b @ b) if st.free and float(b @ b) > 0 else 1.0
    return any(abs(float(a[i] - c * b[i])) > 2 * max(1.0, abs(c)) * float(st.e_d[j]) + 6 * U * abs(float(x[j]))
               for i, j in enumerate(inside))


def _generated(name, n, m, own, bug=None):
    """(report, touched) of the generator on the first four traced problems of a row"""
    key = (name, n, m, own, bug)
    if key in _GENERATED:
        return _GENERATED[key]
    _, lower, upper, x0 = Bc.case(name, n, m, own)
    fun = _numpy_objective(name, n)
    total, touched = Bs.Report(), False
    for b in Bc.TRACED[:4]:
        changes = [] if bug else None
        xs, gs, _ = Bs.generate(fun, x0[b], lower[b], upper[b], m, Bc.limit(m), Bc.GRADIENT_NORM, bug=bug, changes=changes)
        steps = []
        rep = Bs.audit_problem(xs, gs, Bc.rules("generator", m, lower[b], upper[b]), keep=steps,
                               what="generator %s n=%d m=%d problem %d" % (name, n, m, b))
        total.merge(rep)
        for k, st in enumerate(steps if bug else ()):
            touched = touched or _shows(changes[k], xs[k], xs[k + 1], lower[b], upper[b], st)
    _GENERATED[key] = (total, touched)
    return _GENERATED[key]


def test_generator_without_a_bug_is_inside_the_bound_and_the_caps():
    total = Bs.Report()
    for name, n, m, own in Bc.GENERATOR_ROWS:
        rep, _ = _generated(name, n, m, own)
        _assert_case(rep, m, "generator %s n=%d m=%d" % (name, n, m))
        total.merge(rep)
    assert all(c > 0 for c in total.counts()[:5]) and total.evictions > 0, total.line()
    LINES.append("L-BFGS-B step audit, generator: %s" % total.line())


@pytest.mark.parametrize("bug", Bs.BUGS)
def test_a_planted_bug_lands_outside(bug):
    """outside = a coordinate past its bound, on every row the bug touches"""
    seen = 0
    for name, n, m, own in Bc.GENERATOR_ROWS:
        rep, touched = _generated(name, n, m, own, bug)
        if not touched:
            continue
        assert rep.bad or Bs.caps(rep, m), "%s: not seen on %s n=%d m=%d (%s)" % (bug, name, n, m, rep.line())
        seen += 1
    assert seen >= (1 if bug == Bs.STORE_ANYWAY else 2), bug


# ---- 3. every CPU twin trajectory is inside the bound and both caps ---------------------------------------------------------------
def _assert_case(report, m, what):
    line = "%s: %s" % (what, report.line())
    assert not report.bad, "%s\n%d outside their bound, first: %s" % (line, len(report.bad), report.bad[:3])
    broken = Bs.caps(report, m)
    assert not broken, "%s\n%s\nundecidable: %s" % (line, broken, report.undecidable[:4])
    return line


def _twin_report(oracle, family, name, n, m, own, linesearch="more_thuente", traced=Bc.TRACED):
    blob, lower, upper, x0 = Bc.case(name, n, m, own)
    total = Bs.Report()
    for b in traced:
        if family == "relaxed":
            solve = lambda rows, fields: oracle.lbfgsb_fast_minimize_batch(name, rows, m=m, stop=oracle.make_stop(**fields),
                                                                           params=blob, lower=lower[b], upper=upper[b])
        else:
            solve = lambda rows, fields: oracle.lbfgsb_minimize_batch(name, rows, m=m, stop=oracle.make_stop(**fields),
                                                                      params=blob, lower=lower[b], upper=upper[b],
                                                                      reduction="sequential", linesearch=linesearch)
        f0, g0 = oracle.evaluate(name, x0[b], params=blob)
        xs, gs, _ = Bc.prefix_trajectories(solve, x0[b:b + 1], np.array([f0]), np.array([g0]), m)[0]
        total.merge(Bs.audit_problem(xs, gs, Bc.rules(family, m, lower[b], upper[b], linesearch),
                                     what="%s %s n=%d m=%d problem %d" % (family, name, n, m, b)))
    return total


@pytest.mark.parametrize("name,n,m,own", Bc.CPU_ROWS)
def test_reference_order_twin_is_inside_and_runs_every_branch(oracle, name, n, m, own):
    """the reference-order twin (the compiled reference bit for bit: tests/test_oracle.py): the bound, both caps, and the
    inputs do exercise the step — (a)-(e) positive, (a) on at least a tenth of the audited iterations (n = 2: (a), (d), (e),
    tests/bstep_cases.py)"""
    rep = _twin_report(oracle, "reference", name, n, m, own)
    what = "reference-order twin %s n=%d m=%d %s" % (name, n, m, "own boxes" if own else "shared box")
    LINES.append("L-BFGS-B step audit, %s" % _assert_case(rep, m, what))
    assert all(c > 0 for i, c in enumerate(rep.counts()[:5]) if n > 2 or i in (0, 3, 4)), rep.line()
    assert 10 * rep.crossed_with_history >= rep.audited, rep.line()


@pytest.mark.parametrize("name,n,m,own", Bc.CPU_ROWS)
def test_relaxed_twin_is_inside(oracle, name, n, m, own):
    """the relaxed kernel's twin, held to the bound the reference fixed: it enters no calibration"""
    rep = _twin_report(oracle, "relaxed", name, n, m, own)
    what = "relaxed twin %s n=%d m=%d %s" % (name, n, m, "own boxes" if own else "shared box")
    LINES.append("L-BFGS-B step audit, %s" % _assert_case(rep, m, what))


@pytest.mark.parametrize("family,name,n,m,own", [("reference",) + r for r in Bc.E8_ROWS]
                         + [("relaxed",) + r for r in Bc.E8_ROWS if r[1] <= 128])
def test_twins_of_the_wide_rows_are_inside(oracle, family, name, n, m, own):
    """n = 100, 200 (eight coordinates per lane on the device), three traced problems; the relaxed kernel and its twin
    are built up to n = 128"""
    rep = _twin_report(oracle, family, name, n, m, own, traced=Bc.E8_TRACED)
    LINES.append("L-BFGS-B step audit, %s" % _assert_case(rep, m, "%s twin %s n=%d m=%d" % (family, name, n, m)))
    if family == "reference":
        assert all(c > 0 for c in rep.counts()[:5]) and 10 * rep.crossed_with_history >= rep.audited, rep.line()


def test_hager_zhang_reference_order_twin_is_inside(oracle):
    name, n, m, own = Bc.HZ_ROW
    rep = _twin_report(oracle, "reference", name, n, m, own, linesearch="hager_zhang")
    LINES.append("L-BFGS-B step audit, %s" % _assert_case(rep, m, "reference-order twin, Hager-Zhang, %s n=%d m=%d" % (name, n, m)))
