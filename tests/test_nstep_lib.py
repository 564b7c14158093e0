"""tests/nstep_lib.py on the CPU: the replay checks itself, every CPU twin trajectory of tests/nstep_cases.py passes every check
inside both caps (the reference-order twins, which the golden files hold to the compiled reference bit for bit, among them:
the reference measured against the bounds) and runs the branches its row is there for, and a plain generator of each step
that carries a planted bug lands outside.

One line per case goes to the terminal summary (conftest._SUMMARY_LINES); DESIGN.md section 5 carries the table.
"""
import numpy as np
import pytest

import fo_lib
import hp_lib as hp
import nd_lib
import nstep_cases as Nc
import nstep_lib as Ns
import step_cases as Sc
import step_lib as St
import tr_lib

mp, mpf = hp.mp, hp.mpf
TOL = mpf(10) ** -40
LINES = []
ORDERS = {"reference": 0, "exact": 1}        # REF_ORDER, DEVICE_ORDER of the three twin libraries
METHOD = {"gradient_descent": fo_lib.GRADIENT_DESCENT, "conjugated_gradient": fo_lib.CONJUGATED_GRADIENT_DESCENT}


@pytest.fixture(scope="module", autouse=True)
def _lines_to_the_terminal_summary():
    yield
    import conftest
    conftest._SUMMARY_LINES.extend(LINES)


# ---- 1. the replay checks itself -------------------------------------------------------------------------------------------
def _spd(n, seed):
    rng = np.random.default_rng(seed)
    Q = rng.normal(size=(n, n))
    A = Q.T @ Q + np.eye(n)
    A = (A + A.T) / 2
    return [hp.vec(r) for r in A], [[abs(v) for v in hp.vec(r)] for r in A], hp.vec(rng.normal(size=n))


def test_steihaug_with_a_wide_radius_and_no_tolerance_is_the_newton_step():
    """n CG iterations on an SPD model inside a radius that never binds end on -H^-1 g"""
    for n in (3, 7):
        H, H_abs, g = _spd(n, n)
        p, e_p, hit, iters, how = Ns.steihaug(H, H_abs, g, mpf(10) ** 6, mpf(0), mpf(0), n, 4, mpf(0), 1)
        newton = mp.lu_solve(mp.matrix(H), -mp.matrix(g))
        assert not hit and iters == n and how in ("cg_tolerance", "cg_cap")
        assert all(abs(p[j] - newton[j]) <= TOL * max(abs(v) for v in newton) for j in range(n))


def test_steihaug_first_iterate_is_the_cauchy_point_and_the_boundary_step_has_the_radius():
    n = 6
    H, H_abs, g = _spd(n, 3)
    gg, gHg = mp.fdot(g, g), mp.fdot(g, Ns.matvec(H, g))
    p, _, hit, iters, how = Ns.steihaug(H, H_abs, g, mpf(10) ** 6, mpf(0), mpf(0), 1, 4, mpf(0), 1)
    assert (iters, how) == (1, "cg_cap") and all(abs(p[j] + gg / gHg * g[j]) <= TOL for j in range(n))
    radius = mp.sqrt(gg) * gg / gHg / 3
    p, _, hit, iters, how = Ns.steihaug(H, H_abs, g, radius, mpf(0), mpf(0), n, 4, mpf(0), 1)
    assert hit and how == "cg_boundary" and abs(hp.norm2(p) - radius) <= TOL * radius
    assert all(abs(p[j] + radius / mp.sqrt(gg) * g[j]) <= TOL for j in range(n))
    Hn = [[-v for v in r] for r in H]                       # negative curvature: straight to the boundary along -g
    p, _, hit, iters, how = Ns.steihaug(Hn, H_abs, g, radius, mpf(0), mpf(0), n, 4, mpf(0), 1)
    assert hit and (iters, how) == (1, "cg_negative") and abs(hp.norm2(p) - radius) <= TOL * radius


def test_solve_is_the_200_bit_solve_and_its_magnitudes_bound_the_inverse():
    n = 9
    H, _, g = _spd(n, 5)
    solve = Ns.Solve(H)
    want = mp.lu_solve(mp.matrix(H), mp.matrix(g))
    got = solve(g)
    assert all(abs(got[j] - want[j]) <= TOL * max(abs(v) for v in want) for j in range(n))
    inverse = mp.inverse(mp.matrix(H)).tolist()
    assert all(abs(inverse[i][j]) <= solve.ainv[i][j] for i in range(n) for j in range(n))
    assert all(abs(H[i][j]) <= solve.LU[i][j] * (1 + mpf(10) ** -5) for i in range(n) for j in range(n))


def test_dense_quartic_definition_differentiates_itself():
    """g and H of hp_lib.dense_quartic against central differences of its own f and g at 200 bits (a symmetric S: the
    functor's g = S x - b + kappa x^3 is the gradient of its f for those)"""
    n = 5
    rng = np.random.default_rng(4)
    S, b, x = rng.normal(size=(n, n)), rng.normal(size=n), rng.normal(size=n)
    S = (S + S.T) / 2
    ev = hp.dense_quartic(x, S, b, 1.5, hessian=True)
    h = mpf(2) ** -60

    def at(j, sign):
        Sx = [hp.vec(r) for r in S]
        v = hp.vec(x)
        v[j] += sign * h
        return hp._dense_quartic(hp._PLAIN, v, Sx, hp.vec(b), mpf(1.5), hessian=False)

    for j in range(n):
        (fp, gp, _), (fm, gm, _) = at(j, 1), at(j, -1)
        assert abs((fp - fm) / (2 * h) - ev.g[j]) <= mpf(10) ** -30
        for i in range(n):
            assert abs((gp[i] - gm[i]) / (2 * h) - ev.H[i][j]) <= mpf(10) ** -30
    assert all(abs(ev.g[j]) <= ev.g_abs[j] for j in range(n)) and abs(ev.f) <= ev.f_abs


# ---- 2. every CPU twin, reference order and device order --------------------------------------------------------------------
def _start_values(solver, row, x0, order, width=None):
    """f(x_0), g(x_0) as the twin under audit evaluates them: one iteration of that twin under a config whose step is x_0
    itself, so that what it returns is its own evaluation at x_0 (asserted: x comes back unchanged).
      trust region    no retry allowed: the step stalls at once and the prologue's evaluation is returned
      Newton descent  safe_guard = inf: d = -(H + inf I)^-1 g = 0, the first trial is x_0 and is accepted (cache = 0)
      first order     the Fletcher-Reeves twin (the library both methods' evaluations come from) with c = 1e300, rho = 0: the
                      unit trial fails, alpha becomes 0, the trial x_0 + 0 d is accepted and evaluated"""
    oid, blob, _, _, _ = Nc.inputs(row)
    once = Sc.first_iteration_fields()
    if solver == "trust_region":
        x, f, g, p = tr_lib.twin_solve(oid, x0, blob, tr_lib.make_stop(**once), tr_lib.make_config(rejection_retry_limit=0),
                                       order=order)
    elif solver == "newton_descent":
        x, f, g, p = nd_lib.twin_solve(oid, x0, blob, nd_lib.make_stop(**once), nd_lib.make_config(safe_guard=np.inf),
                                       order=order)
    else:
        x, f, g, p = fo_lib.twin_solve(fo_lib.CONJUGATED_GRADIENT_DESCENT, oid, x0, blob, fo_lib.make_stop(**once),
                                       fo_lib.make_config(c=1e300, rho=0.0), order=order, width=width)
    assert np.array_equal(x, x0) and np.isfinite(f).all() and np.isfinite(g).all(), "%s: not the evaluation at x_0" % solver
    return f, g


def _twin_solver(solver, row, order, width=None):
    oid, blob, _, _, _ = Nc.inputs(row)
    config = dict(row[3] or ())
    if solver == "trust_region":
        return lambda rows, fields: tr_lib.twin_solve(oid, rows, blob, tr_lib.make_stop(**fields),
                                                      tr_lib.make_config(**config), order=order)
    if solver == "newton_descent":
        return lambda rows, fields: nd_lib.twin_solve(oid, rows, blob, nd_lib.make_stop(**fields), nd_lib.make_config(),
                                                      order=order)
    return lambda rows, fields: fo_lib.twin_solve(METHOD[solver], oid, rows, blob, fo_lib.make_stop(**fields),
                                                  fo_lib.make_config(), order=order, width=width)


def twin_report(solver, row, family, width=None):
    _, _, x0, evaluate, ks = Nc.inputs(row, sequential=(family == "reference"))
    x0 = x0[list(Nc.TRACED)]
    f0, g0 = _start_values(solver, row, x0, ORDERS[family], width)
    trajectories = Nc.prefix_trajectories(_twin_solver(solver, row, ORDERS[family], width), x0, f0, g0,
                                          Nc.limit_of(solver, row), Nc.PROLOGUE_NFEV[solver])
    rules = Nc.rules_of(solver, row, family)
    return rules, Nc.audit_once(trajectories, rules, evaluate, ks, what="%s %s %s" % (solver, family, Nc.case_id(row)))


@pytest.mark.parametrize("family", ["reference", "exact"])
@pytest.mark.parametrize("solver,row", [(s, r) for s in Nc.SOLVERS for r in Nc.rows_of(s)],
                         ids=lambda v: v if isinstance(v, str) else Nc.case_id(v))
def test_twins_are_inside_the_bounds_and_the_caps(solver, row, family):
    """reference: the reference's own order (the compiled reference bit for bit: the reference measured against the bounds),
    where the row's branches must have run; exact: the kernels' twin at the library's mapping"""
    rules, rep = twin_report(solver, row, family)
    LINES.append("step audit, %s" % Nc.assert_case(rep, rules, "twin %s %s %s" % (family, solver, Nc.case_id(row))))
    if family == "reference":
        missing = [b for b in Nc.required_branches(solver, row) if not getattr(rep, b) > 0]
        assert not missing, "%s %s: branches not exercised: %s (%s)" % (solver, Nc.case_id(row), missing, rep.line())


@pytest.mark.parametrize("solver", ["conjugated_gradient", "gradient_descent"])
@pytest.mark.parametrize("row", Nc.MAPPING_SHAPES, ids=Nc.case_id)
def test_first_order_twins_of_every_padded_width_are_inside(solver, row):
    """the device-order twin at every padded width W x E a built mapping gives n"""
    widths = sorted({W * E for W, E in Nc.mappings_of(row[2])} - {fo_lib.padded_width(row[2])})
    assert widths or row[2] == 256            # (n = 256 has the one mapping, 64 x 4: the library's)
    for width in widths:
        rules, rep = twin_report(solver, row, "exact", width=width)
        LINES.append("step audit, %s" % Nc.assert_case(rep, rules, "twin exact width %d %s %s" % (width, solver,
                                                                                                  Nc.case_id(row))))


# ---- 3. the generators without a bug pass; with a planted bug they do not ---------------------------------------------------
def _numpy_objective(row):
    """(fun(x) -> (f, g), hess(x) -> H) in double, a pairwise tree for the value's sum"""
    name, start, n, _ = row
    if name == "rosenbrock":
        def fun(x):
            t1, t2 = 1.0 - x[:-1], x[1:] - x[:-1] * x[:-1]
            g = np.zeros(n)
            g[:-1] += -2.0 * t1 - 400.0 * x[:-1] * t2
            g[1:] += 200.0 * t2
            return St.tree_dot(np.ones(n - 1), t1 * t1 + 100.0 * t2 * t2), g

        def hess(x):
            H = np.zeros((n, n))
            i = np.arange(n - 1)
            H[i, i] += 1200.0 * x[:-1] * x[:-1] - 400.0 * x[1:] + 2.0
            H[i + 1, i + 1] += 200.0
            H[i, i + 1] = H[i + 1, i] = -400.0 * x[:-1]
            return H
        return fun, hess
    if name == "diag_quadratic":
        a, c = Sc.diag_coefficients(n)
        return (lambda x: (St.tree_dot(a * x, x) + c, 2.0 * a * x)), (lambda x: np.diag(2.0 * a))
    _, blob, _, _, _ = Nc.inputs(row)
    S, b, kappa = blob[:n * n].reshape(n, n).T, blob[n * n:n * n + n], blob[-1]

    def fun(x):
        sx = Ns._chain(S, x)
        return (0.5 * St.tree_dot(x, sx) - St.tree_dot(b, x)) + (0.25 * kappa) * St.tree_dot(x * x, x * x), \
            (sx - b) + kappa * (x * x * x)
    return fun, (lambda x: S + np.diag(3.0 * kappa * x * x))


GENERATOR_ROWS = {
    "trust_region": (("rosenbrock", "u2", 7, None), ("rosenbrock", "std", 9, (("initial_radius", Nc.SMALL_RADIUS),)),
                     ("rosenbrock", "u2", 8, (("initial_radius", Nc.LARGE_RADIUS),)), ("dense", "spd", 7, None),
                     ("dense", "indefinite", 7, None), ("diag_quadratic", "u2", 17, None)),
    "newton_descent": (("rosenbrock", "u2", 7, None), ("rosenbrock", "std", 17, None), ("dense", "spd", 7, None),
                       ("diag_quadratic", "u2", 17, None)),
    "conjugated_gradient": (("rosenbrock", "u2", 7, None), ("rosenbrock", "std", 33, None),
                            ("diag_quadratic", "std", 7, None)),
    "gradient_descent": (("rosenbrock", "u2", 7, None), ("rosenbrock", "std", 33, None), ("diag_quadratic", "std", 7, None)),
}
BUGS = {"trust_region": Ns.TR_BUGS, "newton_descent": Ns.ND_BUGS, "conjugated_gradient": Ns.CG_BUGS,
        "gradient_descent": Ns.GD_BUGS}
_GENERATED = {}


def _generated(solver, row, bug=None):
    key = (solver, row, bug)
    if key not in _GENERATED:
        fun, hess = _numpy_objective(row)
        x0 = Nc.inputs(row)[2][list(Nc.TRACED[:4])]
        limit, config = Nc.limit_of(solver, row), dict(row[3] or ())
        if solver == "trust_region":
            out = [Ns.generate_trust_region(fun, hess, x, limit, config, bug=bug) for x in x0]
        elif solver == "newton_descent":
            out = [Ns.generate_newton_descent(fun, hess, x, limit, bug=bug) for x in x0]
        elif solver == "conjugated_gradient":
            out = [Ns.generate_conjugated_gradient(fun, x, limit, bug=bug) for x in x0]
        else:
            out = [Ns.generate_gradient_descent(fun, x, limit, bug=bug) for x in x0]
        _GENERATED[key] = out
    return _GENERATED[key]


def _audit_generated(solver, row, bug=None):
    _, _, _, evaluate, ks = Nc.inputs(row)
    rules = Nc.rules_of(solver, row)
    return rules, Nc.audit_once(_generated(solver, row, bug), rules, evaluate, ks,
                                what="generator %s %s" % (solver, Nc.case_id(row)))


@pytest.mark.parametrize("solver", Nc.SOLVERS)
def test_generator_without_a_bug_is_inside_the_bounds_and_the_caps(solver):
    total = Ns.Report()
    for row in GENERATOR_ROWS[solver]:
        rules, rep = _audit_generated(solver, row)
        Nc.assert_case(rep, rules, "generator %s %s" % (solver, Nc.case_id(row)))
        total.merge(rep)
    assert total.audited > 40
    LINES.append("step audit, generator %s: %s" % (solver, total.line()))


def _same(a, b):
    return len(a) == len(b) and all(p.shape == q.shape and p.tobytes() == q.tobytes() for s, t in zip(a, b)
                                    for p, q in zip(s, t))


# A planted bug TOUCHES a case where it changes the trajectory or its counts at all: a buggy kernel whose every bit and every
# count is the right one cannot be told from the right one by any test.  What each bug leaves untouched, and why:
#   the curvature term dropped or with c / 2: the cache moves, the trial count only where a trial sits between the two caches
#   rho from -g.p alone: rho moves, a decision only where rho sits between the two values
#   the radius grown without `hit`: shows when a later subproblem reaches the wrongly grown radius
#   steps along -g normalised: a positive multiple of -g under both line-search conditions; it shows where a search
#     accepts its first trial (d sum_k = 1), which must be the unit step — on every generator row it touches.  (On the
#     twins and the device few steps accept at once: three of GradientDescent at n = 2.)
# CG-Steihaug stopping one iteration early or late changes d sum_k and p; rows where the replayed stopping test is itself
# undecidable end the audit there: these two must be caught on at least one row, the others on every row they touch
AT_LEAST_ONE_ROW = (Ns.CG_EARLY, Ns.CG_LATE)
# The search that accepts on sufficient decrease alone is asserted on Rosenbrock only, as in tests/test_step_lib.py: on the
# convex quadratic the first trial that meets the decrease condition along -g meets the curvature condition too on all but 1
# of 164 iterations, and the case stays under the cap on line-search exceptions.
ONLY_ON = {Ns.DECREASE_ALONE: "rosenbrock"}


@pytest.mark.parametrize("solver,bug", [(s, b) for s in Nc.SOLVERS for b in BUGS[s]])
def test_a_planted_bug_lands_outside(solver, bug):
    """outside = a step, a count or a condition past its bound, or a case past a cap"""
    touched = caught = 0
    for row in GENERATOR_ROWS[solver]:
        if _same(_generated(solver, row), _generated(solver, row, bug)) or ONLY_ON.get(bug, row[0]) != row[0]:
            continue
        touched += 1
        rules, rep = _audit_generated(solver, row, bug)
        outside = bool(rep.bad) or bool(St.caps(rep, rules.m))
        caught += outside
        if bug not in AT_LEAST_ONE_ROW:
            assert outside, "%s: not seen on %s (%s)" % (bug, Nc.case_id(row), rep.line())
    assert touched >= 1, "%s touches no case" % bug
    assert caught >= 1, "%s: caught on no row" % bug
    LINES.append("step audit, planted bug '%s': outside on %d of the %d cases it touches" % (bug, caught, touched))
