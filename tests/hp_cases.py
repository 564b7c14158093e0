"""The inputs of the mpmath pins (tests/test_hp_lib.py on the CPU twins, tests/test_gpu_objectives_mpmath.py on the device)
and the one audit both run: a value, gradient and Hessian against tests/hp_lib.py's definition and bound.
TEST INFRASTRUCTURE: only tests/ imports this module."""
import functools

import numpy as np

import hp_lib

DIMS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256)
RIDGE_SHAPES = ((9, 8), (40, 24), (128, 64))          # (rows, n): every form
RIDGE_GRAM_SHAPES = ((129, 65), (300, 100))           # the normal-equation forms only
COMPOSITE_DIMS = (2, 7, 33, 64)
RIDGE_LAMBDA = 0.1
FAMILIES = ("uniform", "near_minimiser", "large", "tiny", "alternating", "one_hot_first", "one_hot_last", "eighths")
ONE_HOT = 0.75     # (not 1: t1 = 1 - x must not vanish at the coordinate the row isolates)


def inputs(n, dtype="float64", seed=0):
    """One row per family, FAMILIES order: [8, n] in `dtype`."""
    rng = np.random.default_rng(1000 * n + seed)
    j = np.arange(n)
    rows = [rng.uniform(-2.0, 2.0, n),
            1.0 + 1e-7 * rng.normal(size=n),                                   # cancellation in t1, t2
            1e3 * rng.normal(size=n),
            (1e-160 if dtype == "float64" else 1e-20) * rng.normal(size=n),    # products underflow
            np.where(j % 2 == 0, 1.5, -1.5),
            np.where(j == 0, ONE_HOT, 0.0),                                    # isolates the first term
            np.where(j == n - 1, ONE_HOT, 0.0),                                # ... and the last
            j / 8.0]                                                           # distinct and exact: a swapped lane shows
    return np.ascontiguousarray(np.array(rows), dtype=np.float32 if dtype == "float32" else np.float64)


def diag_coefficients(n, dtype="float64"):
    """(a, c): both signs, c != 0; in float32 the values the float kernel holds (converted once on upload)"""
    rng = np.random.default_rng(77 + n)
    a = rng.uniform(0.5, 100.0, n) * np.where(np.arange(n) % 3 == 2, -1.0, 1.0)
    c = 5.0
    if dtype == "float32":
        a = a.astype(np.float32).astype(np.float64)
    return a, c


def ridge_data(rows, n, seed=0):
    """A [rows, n], Y [8, rows], X [8, n] (the input families at unit scale where the family is a scale)"""
    rng = np.random.default_rng(31 * rows + n + seed)
    A = rng.normal(size=(rows, n)) / np.sqrt(rows)
    Y = rng.normal(size=(len(FAMILIES), rows))
    return A, Y, inputs(n)


def ridge_own_data(rows, n):
    """one matrix per problem: As [8, rows, n], Y [8, rows], X [8, n]"""
    rng = np.random.default_rng(17 * rows + n)
    return rng.normal(size=(len(FAMILIES), rows, n)) / np.sqrt(rows), rng.normal(size=(len(FAMILIES), rows)), inputs(n)


# ---- the composite: 0 ... 4 constraints of each kind over the whole menu --------------------------------------------------
def composite_terms(n, n_eq, n_ineq, seed=0):
    """[objective] + equalities + inequalities as (prims, form, k, product) with prims (kind, a, c): every kind, every
    form, sums of two and three primitives and a product, within the table's 16 rows."""
    rng = np.random.default_rng(100 * n + 10 * n_eq + n_ineq + seed)
    a = lambda lo=-1.0, hi=1.0: rng.uniform(lo, hi, n)
    objective = ([("rosenbrock", None, 0.0), ("diag_quadratic", a(0.1, 0.5), 0.25)], "plain", 0.0, False)
    eq_menu = [([("linear", a(), 0.0)], "value_minus_k", 0.5, False),
               ([("squared_norm", None, 0.0), ("linear", a(), 0.0)], "k_minus_value", 0.8, False),
               ([("linear", a(0.2, 1.0), 0.0), ("linear", a(0.2, 1.0), 0.0)], "value_minus_k", 0.3, True),
               ([("squared_affine", a(-0.7, 0.7), 0.4)], "plain", 0.0, False)]
    ineq_menu = [([("squared_norm", None, 0.0)], "k_minus_value", 0.5 * n, False),
                 ([("diag_quadratic", a(0.1, 1.0), 1.0), ("linear", a(), 0.0), ("squared_affine", a(-0.5, 0.5), -0.3)],
                  "plain", 0.0, False),
                 ([("linear", a(0.1, 1.0), 0.0), ("diag_quadratic", a(0.1, 1.0), 1.0)], "value_minus_k", 0.2, True),
                 ([("linear", a(), 0.0)], "k_minus_value", 0.1, False)]
    return [objective] + eq_menu[:n_eq] + ineq_menu[:n_ineq]


def composite_case(n, n_eq, n_ineq):
    """terms, X [8, n], lambda [8, n_eq], mu [8, n_ineq], rho [8].  Row 0's first inequality (0.5 n - |x|^2, positive on
    that row) sits on the kink of its max(0, .): mu = rho g(x) + 5e-13, so mu - rho g is within 1e-12 of zero — both
    branches are continuous there, and the bound must hold whichever the device takes."""
    terms = composite_terms(n, n_eq, n_ineq)
    rng = np.random.default_rng(7 * n + n_eq + 5 * n_ineq)
    X = inputs(n)
    X[0] *= 0.25     # (uniform(-0.5, 0.5): inside the ball of the first inequality)
    lam, mu = rng.uniform(-1.0, 1.0, (len(X), n_eq)), rng.uniform(0.0, 2.0, (len(X), n_ineq))
    rho = rng.uniform(0.5, 5.0, len(X))
    if n_ineq:
        g0 = hp_lib.composite(X[0], [terms[1 + n_eq]], 0, [], [], 1.0).f   # the first inequality's own value g(x)
        assert g0 > 0
        mu[0, 0] = rho[0] * float(g0) + 5e-13
        assert abs(hp_lib.mpf(float(mu[0, 0])) - hp_lib.mpf(float(rho[0])) * g0) <= hp_lib.mpf(10) ** -12
    return terms, X, lam, mu, rho


# ---- definitions, evaluated once per (objective, n, dtype) and shared by every mapping -------------------------------------
@functools.lru_cache(maxsize=None)
def rosenbrock_reference(n, dtype="float64", hessian=False):
    return [hp_lib.rosenbrock(x, hessian=hessian) for x in inputs(n, dtype)]


@functools.lru_cache(maxsize=None)
def diag_quadratic_reference(n, dtype="float64", hessian=False):
    a, c = diag_coefficients(n, dtype)
    return [hp_lib.diag_quadratic(x, a, c, hessian=hessian) for x in inputs(n, dtype)]


@functools.lru_cache(maxsize=None)
def ridge_reference(rows, n):
    A, Y, X = ridge_data(rows, n)
    R = hp_lib.Ridge(A, RIDGE_LAMBDA)
    return R, [R(X[b], Y[b]) for b in range(len(X))]


@functools.lru_cache(maxsize=None)
def ridge_own_reference(rows, n):
    As, Y, X = ridge_own_data(rows, n)
    return [hp_lib.Ridge(As[b], RIDGE_LAMBDA)(X[b], Y[b]) for b in range(len(X))]


@functools.lru_cache(maxsize=None)
def composite_reference(n, n_eq, n_ineq):
    terms, X, lam, mu, rho = composite_case(n, n_eq, n_ineq)
    return [hp_lib.composite(X[b], terms, n_eq, lam[b], mu[b], rho[b]) for b in range(len(X))]


# ---- the audit ----------------------------------------------------------------------------------------------------------
class Worst:
    """the worst error-to-bound ratio seen per label; the lines go to the terminal summary"""

    def __init__(self):
        self.ratio = {}

    def see(self, label, ratio):
        self.ratio[label] = max(self.ratio.get(label, 0.0), float(ratio))

    def line(self, title):
        return title + ": " + ", ".join("%s %.3g" % (k, v) for k, v in sorted(self.ratio.items()))


class Reports:
    """The worst ratios of a test module, merged per title; `append_to_summary` (called once, when the module's last test
    has run: a module-scoped fixture of the test file) appends one line per title to conftest._SUMMARY_LINES."""

    def __init__(self):
        self.by_title = {}

    def report(self, title, worst):
        merged = self.by_title.setdefault(title, Worst())
        for label, ratio in worst.ratio.items():
            merged.see(label, ratio)

    def append_to_summary(self):
        import conftest
        for title, merged in self.by_title.items():
            conftest._SUMMARY_LINES.append(merged.line(title))
        self.by_title = {}


def audit(ev, f, g, ks, dtype="float64", H=None, worst=None, label="", what=""):
    """f, g[j] (and H[i][j], already transposed to row i / column j) against the definition `ev` under ks = (k_f, k_g[,
    k_H]).  Returns the list of violations (empty: inside the bound everywhere)."""
    bad = []

    def one(name, value, definition, k, magnitude):
        ok, ratio = hp_lib.within(value, definition, k, magnitude, dtype)
        if worst is not None and ratio != hp_lib.mp.inf:
            worst.see(label + name[0], ratio)
        if not ok:
            bad.append("%s %s: got %r, definition %s, ratio %s" % (what, name, float(value), hp_lib.mp.nstr(definition, 20),
                                                                   hp_lib.mp.nstr(ratio, 5)))

    one("f", f, ev.f, ks[0], ev.f_abs)
    for j in range(len(ev.g)):
        one("g[%d]" % j, g[j], ev.g[j], ks[1], ev.g_abs[j])
    if H is not None:
        n = len(ev.g)
        for i in range(n):
            for j in range(n):
                one("H[%d][%d]" % (i, j), H[i][j], ev.H[i][j], ks[2], ev.H_abs[i][j])
    return bad


# ---- what a solver returns ------------------------------------------------------------------------------------------------
STATUS_ITERATION_LIMIT, STATUS_GRADIENT_NORM = 1, 4     # cppoptlib::solver::Status (solver/progress.h)
RESULT_B = 24
RESULT_DIMS = (2, 7, 33, 64)
MAX_BAILOUTS_OF_24 = 2     # at most 2 of 24 problems of a batch may end non-finite; a smaller batch in proportion


def max_bailouts(B):
    return MAX_BAILOUTS_OF_24 * B // RESULT_B


def result_starts(objective, n, B=RESULT_B):
    """the seeds of tests/at_lib.py's starts, no hostile rows"""
    import at_lib
    return at_lib.starts(objective, B, n, seed=4100 + n)


def result_diag_coefficients(n, dtype="float64"):
    """a > 0 (strongly convex: mu = 2 min a), c = 0.25"""
    import at_lib
    p = at_lib.diag_params(n)
    if dtype == "float32":
        p = p.astype(np.float32).astype(np.float64)
    return p[:-1], float(p[-1])


def result_box(n, per_problem=False):
    """a box that cuts the Rosenbrock minimiser (1, ..., 1) off and leaves the quadratic's inside; one per problem: the same
    box moved by up to 0.1"""
    lower, upper = np.full(n, -0.5), np.full(n, 0.8)
    if per_problem:
        shift = 0.1 * np.random.default_rng(n).uniform(0.0, 1.0, (RESULT_B, 1))
        return lower - shift, upper + shift
    return lower, upper


def audit_results(evaluate, ks, x0, x, f, g, progress, stop, dtype="float64", value_only=False, lower=None, upper=None,
                  lbfgsb=False, minimiser=None, mu=None, worst=None, label="", what=""):
    """The postconditions of a finished batch that hold for any correct solver.  evaluate(b, row) -> hp_lib.Eval of
    problem b at `row` (the exact values returned).  progress: numpy records.  Returns (violations, excluded): a problem
    that ended on a non-finite bail-out is excluded from the value checks and counted.

      * f and g are the objective's value and gradient at the returned x, within the bounds of hp_lib (value_only: f)
      * progress.gradient_norm == max_j |g_j| of the returned g, exactly.  (Also under Lbfgsb: the field is written by
        Progress::Update from the full gradient of the returned iterate.  The box-projected sup norm — |g_j| dropped where
        x_j sits on a bound and g_j points out of the box — is what Lbfgsb's stopping test reads, at the iterate the last
        step STARTED from and against the plain tolerance; that iterate is not returned, so for Lbfgsb (lbfgsb=True)
        the implication below is not asserted.)
      * status GRADIENT_NORM implies gradient_norm < tol * (max(1, ||x||_inf) if relative else 1)
      * status ITERATION_LIMIT implies num_iterations > limit
      * f(x) <= f(x0), both sides at 200 bits
      * lower <= x <= upper, exactly
      * strongly convex objectives: ||x - x*||_2 <= ||grad f(x)||_2 / mu * (1 + 1e-9), an inequality of the mathematics
    """
    bad, excluded = [], 0
    mp, mpf = hp_lib.mp, hp_lib.mpf
    boxed = lower is not None
    for b in range(x.shape[0]):
        tag = "%s problem %d" % (what, b)
        status, iterations = int(progress["status"][b]), int(progress["num_iterations"][b])
        if status == STATUS_ITERATION_LIMIT and not iterations > stop.num_iterations:
            bad.append("%s: ITERATION_LIMIT after %d of %d iterations" % (tag, iterations, stop.num_iterations))
        if status <= 0:
            bad.append("%s: status %d on a finished problem" % (tag, status))
        if boxed:
            lo, hi = (lower if lower.ndim == 1 else lower[b]), (upper if upper.ndim == 1 else upper[b])
            if not (np.all(lo <= x[b]) and np.all(x[b] <= hi)):
                bad.append("%s: x leaves its box" % tag)
        finite = np.isfinite(x[b]).all() and np.isfinite(f[b]) and (value_only or np.isfinite(g[b]).all())
        if not finite:
            excluded += 1
            continue
        ev = evaluate(b, x[b])
        if value_only:
            bad += _audit_value(ev, f[b], ks, dtype, worst, label, tag)
        else:
            bad += audit(ev, f[b], g[b], ks, dtype=dtype, worst=worst, label=label, what=tag)
        if not value_only:
            gn = float(progress["gradient_norm"][b])
            if gn != float(np.max(np.abs(g[b].astype(np.float64)))):
                bad.append("%s: gradient_norm %r is not max|g_j| %r" % (tag, gn, float(np.max(np.abs(g[b])))))
            if status == STATUS_GRADIENT_NORM and not lbfgsb:
                scale = max(1.0, float(np.max(np.abs(x[b].astype(np.float64))))) if stop.gradient_norm_relative else 1.0
                if not gn < stop.gradient_norm * scale:
                    bad.append("%s: GRADIENT_NORM with gradient_norm %r, tolerance %r"
                               % (tag, gn, stop.gradient_norm * scale))
        f0 = evaluate(b, x0[b]).f
        if not ev.f <= f0:
            bad.append("%s: f(x) = %s above f(x0) = %s" % (tag, mp.nstr(ev.f, 20), mp.nstr(f0, 20)))
        if minimiser is not None:
            xs = minimiser(b)
            distance = hp_lib.norm2([mpf(float(v)) - s for v, s in zip(x[b], xs)])
            if not distance <= hp_lib.norm2(ev.g) / mu * (1 + mpf(10) ** -9):
                bad.append("%s: %s from the minimiser with a gradient of %s, mu %s" % (
                    tag, mp.nstr(distance, 8), mp.nstr(hp_lib.norm2(ev.g), 8), mp.nstr(mu, 8)))
    if excluded > max_bailouts(x.shape[0]):
        bad.append("%s: %d of %d problems ended non-finite" % (what, excluded, x.shape[0]))
    return bad, excluded


def _audit_value(ev, f, ks, dtype, worst, label, tag):
    ok, ratio = hp_lib.within(f, ev.f, ks[0], ev.f_abs, dtype)
    if worst is not None and ratio != hp_lib.mp.inf:
        worst.see(label + "f", ratio)
    return [] if ok else ["%s f: got %r, definition %s, ratio %s" % (tag, float(f), hp_lib.mp.nstr(ev.f, 20),
                                                                    hp_lib.mp.nstr(ratio, 5))]


def memo(fn):
    """evaluate(b, row) remembered by the row's bytes: the starts are shared by every solver of a test"""
    seen = {}

    def evaluate(b, row):
        key = (b, row.dtype.str, row.tobytes())
        if key not in seen:
            seen[key] = fn(b, row)
        return seen[key]
    return evaluate


@functools.lru_cache(maxsize=None)
def result_objective(name, n, dtype="float64"):
    """(params, evaluate, ks, minimiser, mu) of "rosenbrock" / "diag_quadratic" for the result audits; params is what
    amd.DiagQuadratic takes, (a, c), or None"""
    if name == "rosenbrock":
        return None, memo(lambda b, row: hp_lib.rosenbrock(row)), hp_lib.rosenbrock_k(n), None, None
    a, c = result_diag_coefficients(n, dtype)
    zero = [hp_lib.mpf(0)] * n
    return ((a, c), memo(lambda b, row: hp_lib.diag_quadratic(row, a, c)), hp_lib.diag_quadratic_k(n), lambda b: zero,
            2 * hp_lib.mpf(float(a.min())))


RIDGE_RESULT_SHAPES = ((40, 24), (128, 64))


@functools.lru_cache(maxsize=None)
def ridge_result_case(rows, n):
    """A, Y [B, rows], x0 and (evaluate, ks, minimiser, mu = 2 lam) of the shared-matrix forms"""
    rng = np.random.default_rng(5 * rows + n)
    A, Y = rng.normal(size=(rows, n)) / np.sqrt(rows), rng.normal(size=(RESULT_B, rows))
    R = hp_lib.Ridge(A, RIDGE_LAMBDA)
    return (A, Y, result_starts("ridge", n), memo(lambda b, row: R(row, Y[b])), R.k(), lambda b: R.minimiser(Y[b]),
            2 * R.lam)


@functools.lru_cache(maxsize=None)
def ridge_own_result_case(rows, n, B=8):
    """one matrix per problem: As, Y, x0 and (evaluate, ks, minimiser, mu = 2 lam).  A batch of 8, with no bail-out
    allowed (max_bailouts): every problem converts its own matrix to mpf and factors its own normal equations."""
    rng = np.random.default_rng(9 * rows + n)
    As, Y = rng.normal(size=(B, rows, n)) / np.sqrt(rows), rng.normal(size=(B, rows))
    Rs = [hp_lib.Ridge(As[b], RIDGE_LAMBDA) for b in range(B)]
    return (As, Y, result_starts("ridge", n, B), memo(lambda b, row: Rs[b](row, Y[b])), (n + rows, n + rows),
            lambda b: Rs[b].minimiser(Y[b]), 2 * Rs[0].lam)


COMPOSITE_RESULT_COUNTS = (2, 2)     # equalities, inequalities of the composite the result audits solve


@functools.lru_cache(maxsize=None)
def composite_result_case(n):
    """terms, n_eq, x0 [24, n] (tests/at_lib.py's starts), lambda, mu, rho per problem, evaluate, k"""
    n_eq, n_ineq = COMPOSITE_RESULT_COUNTS
    terms = composite_terms(n, n_eq, n_ineq)
    rng = np.random.default_rng(50 + n)
    x0 = result_starts("composite", n)
    lam, mu = rng.uniform(-1.0, 1.0, (RESULT_B, n_eq)), rng.uniform(0.0, 2.0, (RESULT_B, n_ineq))
    rho = rng.uniform(0.5, 5.0, RESULT_B)
    evaluate = memo(lambda b, row: hp_lib.composite(row, terms, n_eq, lam[b], mu[b], rho[b]))
    return terms, n_eq, x0, lam, mu, rho, evaluate, hp_lib.composite_k(n, terms)


AL_REPORT_CASES = ((2, 1, 1), (7, 2, 2), (33, 1, 2), (64, 2, 1))     # n, equalities, inequalities


def al_report_case(n, n_eq, n_ineq):
    """terms and the 24 starts (tests/at_lib.py's) of the augmented-Lagrangian report audit"""
    return composite_terms(n, n_eq, n_ineq), 0.5 * result_starts("composite", n)


# ---- the augmented-Lagrangian solver's report ------------------------------------------------------------------------------
def audit_al_report(terms, n_eq, x, lam, mu, max_violation, kkt, worst=None, what=""):
    """What BatchedAugmentedLagrangian reports with the state it returns, restated from the reference's
    solver/augmented_lagrangian.h:
      max_violation = max( max_i |c_i(x)| , max_j max(0, -g_j(x)) )                 (OptimizationStep, step 4, :356-387)
      KKT norm      = || grad f + sum_i lambda_i grad c_i - sum_j mu_j grad g_j ||_inf   with the returned multipliers
                                                                              (ComputeLagrangianGradientKktNorm, :577-604)
    each within the rounding bound of its own magnitude: a maximum moves by at most the largest bound of its entries."""
    bad = []
    mp, mpf = hp_lib.mp, hp_lib.mpf
    n = x.shape[1]
    k = hp_lib.composite_k(n, terms)
    for b in range(x.shape[0]):
        if not (np.isfinite(x[b]).all() and np.isfinite(kkt[b]) and np.isfinite(max_violation[b])):
            bad.append("%s problem %d: non-finite report" % (what, b))
            continue
        parts = [hp_lib.composite(x[b], [t], 0, [], [], 1.0) for t in terms]    # every term on its own: value, gradient
        violation, slack = mpf(0), mpf(0)
        for i, ev in enumerate(parts[1:]):
            violation = max(violation, abs(ev.f) if i < n_eq else max(mpf(0), -ev.f))
            slack = max(slack, hp_lib.bound(k, ev.f_abs))
        grad, grad_abs = list(parts[0].g), list(parts[0].g_abs)
        for i, ev in enumerate(parts[1:]):
            w = mpf(float(lam[b][i])) if i < n_eq else -mpf(float(mu[b][i - n_eq]))
            for j in range(n):
                grad[j] += w * ev.g[j]
                grad_abs[j] += abs(w) * ev.g_abs[j]
        for name, got, want, tol in (("max_violation", max_violation[b], violation, slack),
                                     ("KKT norm", kkt[b], max(abs(v) for v in grad),
                                      max(hp_lib.bound(k, m) for m in grad_abs))):
            error = abs(mpf(float(got)) - want)
            if worst is not None and tol > 0:
                worst.see(name + " ", error / tol)
            if not error <= tol:
                bad.append("%s problem %d: %s %r, definition %s" % (what, b, name, float(got), mp.nstr(want, 20)))
    return bad
