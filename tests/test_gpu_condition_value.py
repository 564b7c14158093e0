"""The condition number the solve kernels compute (csrc/hessian_condition_device.hpp), pinned to its VALUE through the
one bit the kernels report: status 5 when `condition > stop.condition_hessian`.

For an iterate x_k of a batch under a stop record in which only the iteration limit is active, the host builds H(x_k) in
the functor's operation order, takes the CPU twin's condition number c, and launches the kernel at the thresholds
lo = c (1 - delta) rounded down and hi = c (1 + delta) rounded up, delta = (2 n^2 + 8) 2^-53 (derived in
tests/cond_cases.py; tests/test_cond_bracket_cpu.py shows what wrong kernels these brackets catch).  The kernel must stop
at x_k on lo (status 5, num_iterations == k, x == x_k bit for bit) and must not on hi.  Every launch carries the whole
batch: the other problems must stop exactly where their own condition numbers say, wherever those are clear of the
threshold by more than delta.

x_k is read from the per-iteration trace of a baseline launch with the test off and the limit at k: it ends with
num_iterations == k + 1 on the limit, so the solve was in status CONTINUE at x_k (a limit of 0 means "no limit", so no
limit returns x_1 itself; for k >= 2 the launch at limit k - 1 returns x_k and must agree with the trace).

Where the Hessian does not depend on x (DiagQuadratic; the dense functor with kappa = 0, whose S the batch shares) the
problems of a batch have one condition number: one bracket, which all of them must obey, each at its own x_1."""
import math
import os

import numpy as np
import pytest

import cond_cases as K
import nd_lib as T
import test_dense_lu_mpmath as L

pytestmark = pytest.mark.gpu

NEWTON = ("newton_descent", "trust_region")
# (line search, arithmetic): the three Lbfgs kernels that carry the LU — exact, fused More-Thuente, Hager-Zhang
LBFGS_VARIANTS = (("more_thuente", "exact"), ("more_thuente", "fma"), ("hager_zhang", "exact"))


@pytest.fixture(scope="module")
def contexts():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import cppnumericalsolvers_amd as amd
    ctx = {"default": amd.Context(0),
           "user": amd.Context(0, library=os.path.join(T.REPO, "cppnumericalsolvers_amd", "libmi355_lbfgs_tr.so"))}
    yield ctx
    for c in ctx.values():
        c.close()


def _twin_condition(solver):
    return L.tr_twin_condition if solver == "trust_region" else T.twin_condition


class Kernel:
    """One solve kernel on one objective: launches of the whole batch at an iteration limit and a threshold."""

    def __init__(self, contexts, solver, objective, x0, user=False, **options):
        import torch
        self.solver, self.objective, self.options = solver, objective, options
        self.ctx = contexts["user" if user else "default"]
        self.x0 = np.ascontiguousarray(x0, dtype=np.float64)
        self.x0_dev = torch.from_numpy(self.x0).to("cuda:0")
        self.launches, self.mapping = 0, None

    def run(self, limit, threshold, trace=False):
        """-> x [B, n], status [B], num_iterations [B] (and the traced iterates [B][k] with trace=True)"""
        import torch
        import cppnumericalsolvers_amd as amd
        from cppnumericalsolvers_amd import capi
        stop = capi.Stop()                      # every test off but the iteration limit
        stop.num_iterations, stop.x_delta_violations, stop.f_delta_violations = int(limit), 1, 1
        cls = {"lbfgs": amd.BatchedLbfgs, "newton_descent": amd.BatchedNewtonDescent,
               "trust_region": amd.BatchedTrustRegionNewton}[self.solver]
        s = cls(stopping_progress=stop, condition_hessian=float(threshold), context=self.ctx, **self.options)
        B, n = self.x0.shape
        t = amd.Trace(np.arange(B), limit + 2, n, "cuda:0") if trace else None
        x, _, _, p = s.minimize(self.objective, self.x0_dev, trace=t)
        torch.cuda.synchronize()
        self.launches += 1
        ll = s.last_launch()
        self.mapping = (ll["lanes_per_problem"], ll["elems_per_lane"])
        self.arithmetic = s.last_arithmetic()
        p = amd.progress_to_numpy(p)
        out = (x.cpu().numpy(), p["status"].copy(), p["num_iterations"].copy())
        if not trace:
            return out
        iterates = []
        for b in range(B):
            rec, xs, _ = t.history(b)
            assert rec["num_iterations"].tolist() == list(range(1, len(rec) + 1)), (b, rec["num_iterations"])
            iterates.append(xs)
        return out + (iterates,)


def _same_rows(a, b):
    return a.tobytes() == b.tobytes()


def _decision(c, t, n):
    """the twin's `c > t`, or None where c is within delta of t (finite c only: inf and NaN decide alone)"""
    if not math.isfinite(c):
        return bool(c > t)
    return bool(c > t) if K.clear_of(c, t, n) else None


def _expected_stop(values, t, n):
    """values: the twin's condition numbers of a problem's iterates 1 .. k.  -> the iterate the kernel stops at on the
    threshold t (0: it runs into the limit), or None where some value on the way is too close to t to say."""
    for k, c in enumerate(values, start=1):
        d = _decision(c, t, n)
        if d is None:
            return None
        if d:
            return k
    return 0


def _assert_launch(kernel, t, limit, values, iterates, n, required, what):
    """One launch at threshold t: every problem stops where `required[b]` (the bracketed ones) or its own condition
    numbers (the others, where clear) say: 0 = on the limit, k = on the condition test at iterate k with x == x_k."""
    x, status, iters = kernel.run(limit, t)
    for b in range(x.shape[0]):
        want = required.get(b, _expected_stop(values[b], t, n))
        if want is None:
            continue
        got = "status %d after %d iterations" % (status[b], iters[b])
        if want == 0:
            assert status[b] == K.ITERATION_LIMIT and iters[b] == limit + 1, \
                "%s: problem %d at threshold %r: %s, expected to run into the limit (twin's values %r)" % (
                    what, b, t, got, values[b])
        else:
            assert status[b] == K.CONDITION and iters[b] == want, \
                "%s: problem %d at threshold %r: %s, expected status 5 at iterate %d (twin's values %r)" % (
                    what, b, t, got, want, values[b])
            assert _same_rows(x[b], iterates[b][want - 1]), "%s: problem %d stopped at another x" % (what, b)


def baseline(kernel, hessian, iterate, what):
    """The generator conditions on the device's own solve, then -> (iterates [B][k], values [B][k], groups): the traced
    x_1 .. x_iterate, the twin's condition numbers of H at each, and the problems grouped by the bytes of H(x_iterate)."""
    n = kernel.x0.shape[1]
    x, status, iters, iterates = kernel.run(iterate, 0.0, trace=True)
    assert (status == K.ITERATION_LIMIT).all() and (iters == iterate + 1).all(), \
        "%s: the baseline does not run past iterate %d on the limit alone: status %s after %s" % (what, iterate, status, iters)
    assert all(len(xs) == iterate + 1 and np.isfinite(xs).all() for xs in iterates), what
    assert all(_same_rows(x[b], iterates[b][iterate]) for b in range(len(iterates))), what
    if iterate >= 2:
        xk, status, iters = kernel.run(iterate - 1, 0.0)
        assert (status == K.ITERATION_LIMIT).all() and (iters == iterate).all(), what
        assert all(_same_rows(xk[b], iterates[b][iterate - 1]) for b in range(len(iterates))), what
    cond = _twin_condition(kernel.solver)
    values = [[cond(hessian(xs[k])) for k in range(iterate)] for xs in iterates]
    groups = {}
    for b, xs in enumerate(iterates):
        groups.setdefault(hessian(xs[iterate - 1]).tobytes(), []).append(b)
    return iterates, values, list(groups.values())


def bracket(kernel, hessian, what, iterate=1, rows=None):
    """The whole procedure on one batch; returns the number of brackets asserted.  rows: the problems to bracket (default:
    all of them); at a later iterate their thresholds must lie above the twin's values at the iterates before it."""
    n = kernel.x0.shape[1]
    iterates, values, groups = baseline(kernel, hessian, iterate, what)
    last = [v[-1] for v in values]
    assert all(math.isfinite(c) and c < K.MAX_CONDITION for c in last), (what, last)
    assert K.separated([last[g[0]] for g in groups], n), "%s: condition numbers within 4 delta: %r" % (what, last)
    if rows is not None:
        groups = [g for g in groups if set(g) & set(rows)]
        assert sorted(b for g in groups for b in g) == sorted(rows), (what, groups, rows)
    done = 0
    for g in groups:
        c = last[g[0]]
        lo, hi = K.thresholds(c, n)
        for b in g:
            # a threshold at or below an earlier value would stop the solve before it reaches the iterate
            assert all(v < lo and K.clear_of(v, lo, n) for v in values[b][:-1]), \
                "%s: problem %d: the lower threshold %r is not above the twin's earlier values %r" % (what, b, lo, values[b])
        _assert_launch(kernel, lo, iterate, values, iterates, n, {b: iterate for b in g}, what + " (lower threshold)")
        _assert_launch(kernel, hi, iterate, values, iterates, n, {b: 0 for b in g}, what + " (upper threshold)")
        done += 1
    return done


def _lbfgs_mappings(n):
    """one coordinate per lane, two per lane"""
    return ((T.padded_width(n), 1), (K.two_row_width(n), 2))


# ---- 1. the three kernels on what they already run ---------------------------------------------------------------------


@pytest.mark.parametrize("linesearch,arithmetic", LBFGS_VARIANTS)
@pytest.mark.parametrize("n", K.ROSENBROCK_DIMS)
def test_lbfgs_rosenbrock(contexts, n, linesearch, arithmetic):
    import cppnumericalsolvers_amd as amd
    ran = set()
    def make(W, E):
        return Kernel(contexts, "lbfgs", amd.Rosenbrock(differentiability="second"), K.rosenbrock_starts(n), m=5,
                      linesearch=linesearch, arithmetic=arithmetic, lanes_per_problem=W, elems_per_lane=E)

    # The library's choice WITH the test on (at most two coordinates per lane then; without it it may take four, and
    # the fused arithmetic's bits depend on that count): read from one launch, and bracketed under its own name unless it
    # is one of the two forced mappings
    probe = make(0, 0)
    probe.run(1, 1.7e308)
    assert probe.mapping[1] <= 2, probe.mapping
    for W, E in dict.fromkeys(_lbfgs_mappings(n) + (probe.mapping,)):
        kernel = make(W, E)
        what = "Lbfgs %s/%s, Rosenbrock n = %d, mapping %d x %d" % (linesearch, arithmetic, n, W, E)
        assert bracket(kernel, K.rosenbrock_hessian, what) == K.B
        assert kernel.launches == 1 + 2 * K.B
        assert kernel.mapping == (W, E), (what, kernel.mapping)
        assert kernel.arithmetic == arithmetic, (what, kernel.arithmetic)
        ran.add(kernel.mapping[1])
    assert ran == {1, 2}, "both coordinates-per-lane counts ran"


def _newton_objectives(amd, n):
    yield "Rosenbrock", amd.Rosenbrock(), K.rosenbrock_starts(n), K.rosenbrock_hessian
    for indefinite in (False, True):
        a, c, x0 = K.diag_quadratic_inputs(n, indefinite)
        yield ("DiagQuadratic (%s)" % ("indefinite" if indefinite else "convex"), amd.DiagQuadratic(a, c), x0,
               lambda x, a=a: K.diag_quadratic_hessian(a))


@pytest.mark.parametrize("solver", NEWTON)
@pytest.mark.parametrize("n,W", K.NEWTON_PAIRS)
def test_newton_kernels_rosenbrock_and_diag_quadratic(contexts, solver, n, W):
    import cppnumericalsolvers_amd as amd
    for name, objective, x0, hessian in _newton_objectives(amd, n):
        kernel = Kernel(contexts, solver, objective, x0, lanes_per_problem=W)
        what = "%s, %s n = %d on %d lanes" % (solver, name, n, W)
        if n == 1 and name == "Rosenbrock":
            # H = (0): the twin's value is NaN and the test never fires, whatever the threshold
            assert math.isnan(_twin_condition(solver)(hessian(x0[0])))
            for t in (1.0, 1.7e308):
                _, status, iters = kernel.run(1, t)
                assert (status == K.ITERATION_LIMIT).all() and (iters == 2).all(), (what, t, status)
            continue
        assert bracket(kernel, hessian, what) == (K.B if name == "Rosenbrock" else 1)
        assert kernel.mapping == (W, 1)


# ---- 2. dense matrices under NewtonDescent and TrustRegionNewton -------------------------------------------------------


def _dense(amd, params):
    return amd.Objective(K.D.DENSE, params, "dense_quartic")


@pytest.mark.parametrize("solver", NEWTON)
@pytest.mark.parametrize("n", K.DENSE_DIMS)
def test_newton_kernels_dense(contexts, solver, n):
    import cppnumericalsolvers_amd as amd
    x0, b = K.dense_starts(n), K.dense_rhs(n)
    for name, S in K.dense_matrices(n):
        if name == K.SINGULAR:
            continue
        p = K.dense_params(S, b, 0.0)
        kernel = Kernel(contexts, solver, _dense(amd, p), x0, user=True)
        assert bracket(kernel, lambda x, p=p: K.dense_hessian(p, x), "%s, dense n = %d, %s" % (solver, n, name)) == 1
    p, x0 = K.kappa_batch(n)
    kernel = Kernel(contexts, solver, _dense(amd, p), x0, user=True)
    assert bracket(kernel, lambda x: K.dense_hessian(p, x), "%s, dense n = %d, kappa = 0.5" % (solver, n)) == K.B


# ---- 3. dense matrices under Lbfgs -------------------------------------------------------------------------------------


def _dense_second(amd, params):
    obj = _dense(amd, params)
    obj.hessian_from_functor = True      # Second mode: hess_diag preconditions, hess_full feeds the condition test
    return obj


@pytest.mark.parametrize("n,E", [(n, 2) for n in K.LBFGS_TWO_ROW_DIMS] + [(n, 1) for n in K.LBFGS_ONE_ROW_DIMS])
def test_lbfgs_dense(contexts, n, E):
    """The LU at two rows of the trailing block per lane and the inverse in two passes, on dense matrices (E = 2:
    n > W at every n here), and the same matrices at one coordinate per lane."""
    import cppnumericalsolvers_amd as amd
    W = K.two_row_width(n) if E == 2 else T.padded_width(n)
    x0, b = K.dense_starts(n), K.dense_rhs(n)
    for linesearch in ("more_thuente", "hager_zhang"):
        for name, S in K.dense_matrices(n):
            if name == K.SINGULAR:
                continue
            p = K.dense_params(S, b, 0.0)
            kernel = Kernel(contexts, "lbfgs", _dense_second(amd, p), x0, user=True, m=5, linesearch=linesearch,
                            arithmetic="exact", lanes_per_problem=W, elems_per_lane=E)
            what = "Lbfgs %s, dense n = %d on %d x %d, %s" % (linesearch, n, W, E, name)
            assert bracket(kernel, lambda x, p=p: K.dense_hessian(p, x), what) == 1
            assert kernel.mapping == (W, E) and (E == 1 or n > W), (what, kernel.mapping)
    p, x0 = K.kappa_batch(n)
    kernel = Kernel(contexts, "lbfgs", _dense_second(amd, p), x0, user=True, m=5, arithmetic="exact",
                    lanes_per_problem=W, elems_per_lane=E)
    assert bracket(kernel, lambda x: K.dense_hessian(p, x), "Lbfgs, dense n = %d on %d x %d, kappa = 0.5" % (n, W, E)) == K.B
    assert kernel.mapping == (W, E)


# ---- 4. edges ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("solver", NEWTON + ("lbfgs",))
@pytest.mark.parametrize("n", (9, 33))
def test_singular_hessian(contexts, solver, n):
    """S with a zero first row and column, kappa = 0: H is singular at every x, the LU takes its `best == 0` branch and
    the substitutions divide by zero.  The twin's value is NaN (0 x inf in the substitutions): `NaN > t` is false, and the
    device must not stop either, at the largest threshold or at 1."""
    import cppnumericalsolvers_amd as amd
    S = dict(K.dense_matrices(n))[K.SINGULAR]
    c = _twin_condition(solver)(S)
    assert not math.isfinite(c)
    p = K.dense_params(S, K.dense_rhs(n), 0.0)
    if solver == "lbfgs":
        kernel = Kernel(contexts, solver, _dense_second(amd, p), K.dense_starts(n), user=True, m=5, arithmetic="exact",
                        lanes_per_problem=K.two_row_width(n), elems_per_lane=2)
    else:
        kernel = Kernel(contexts, solver, _dense(amd, p), K.dense_starts(n), user=True)
    _, status0, iters0 = kernel.run(1, 0.0)
    for t in (1.7e308, 1.0):
        _, status, iters = kernel.run(1, t)
        fired = (status == K.CONDITION) & (iters == 1)
        assert (fired == bool(c > t)).all(), (solver, n, t, c, status, iters)
        if not c > t:     # ... and the test being on changes nothing
            assert (status == status0).all() and (iters == iters0).all(), (solver, n, t, status, status0)


@pytest.mark.parametrize("solver", NEWTON)
def test_infinite_value_fires(contexts, solver):
    """H = diag(1e-160): the inverse's squares overflow, the twin's value is +inf, and inf > t fires at every finite t."""
    import cppnumericalsolvers_amd as amd
    n = 7
    a = np.full(n, 0.5e-160)
    assert _twin_condition(solver)(K.diag_quadratic_hessian(a)) == math.inf
    kernel = Kernel(contexts, solver, amd.DiagQuadratic(a, 0.0), K.rosenbrock_starts(n))
    for t in (1.7e308, 1.0):
        _, status, iters = kernel.run(1, t)
        assert (status == K.CONDITION).all() and (iters == 1).all(), (solver, t, status, iters)


@pytest.mark.parametrize("solver", NEWTON + ("lbfgs",))
def test_later_iterate(contexts, solver):
    """The bracket at iterate 3 (baseline limits 3, traced, and 2) of the rows chosen up front (cond_cases: those whose
    condition number at iterate 3 exceeds the ones at iterates 1 and 2, asserted on the device's own iterates here and on
    the twins' in test_cond_bracket_cpu.py): the LDS region of the LU is intact after the history has grown."""
    import cppnumericalsolvers_amd as amd
    n, x0 = K.LATER_ITERATE_N, K.later_iterate_starts()
    if solver == "lbfgs":
        kernel = Kernel(contexts, solver, amd.Rosenbrock(differentiability="second"), x0, m=5, arithmetic="exact",
                        lanes_per_problem=16, elems_per_lane=2)
    else:
        kernel = Kernel(contexts, solver, amd.Rosenbrock(), x0)
    rows = K.LATER_ITERATE_ROWS[solver]
    assert bracket(kernel, K.rosenbrock_hessian, "%s, Rosenbrock n = %d at iterate 3" % (solver, n), iterate=3,
                   rows=rows) == len(rows)


@pytest.mark.parametrize("solver", NEWTON)
def test_one_dimension_is_exactly_one(contexts, solver):
    """n = 1, H = (4): c = |4| fl(1 / 4) = 1 exactly.  The device fires at t = 1 - 2^-53 and not at t = 1."""
    import cppnumericalsolvers_amd as amd
    a, c, x0 = K.diag_quadratic_inputs(1, False)
    assert _twin_condition(solver)(K.diag_quadratic_hessian(a)) == 1.0
    kernel = Kernel(contexts, solver, amd.DiagQuadratic(a, c), x0, lanes_per_problem=8)
    _, status, iters = kernel.run(1, 1.0 - 2.0 ** -53)
    assert (status == K.CONDITION).all() and (iters == 1).all(), (status, iters)
    _, status, iters = kernel.run(1, 1.0)
    assert (status == K.ITERATION_LIMIT).all() and (iters == 2).all(), (status, iters)


# ---- 6. the device's value itself, for the record ----------------------------------------------------------------------


def _record_kernel(contexts, kind, n, W, E):
    import cppnumericalsolvers_amd as amd
    solver, hessian_kind = kind.split("/")
    mapping = dict(lanes_per_problem=W, elems_per_lane=E, m=5, arithmetic="exact") if solver == "lbfgs" else \
        dict(lanes_per_problem=W)
    if hessian_kind == "rosenbrock":
        second = "second" if solver == "lbfgs" else "first"
        return (Kernel(contexts, solver, amd.Rosenbrock(differentiability=second), K.rosenbrock_starts(n), **mapping),
                K.rosenbrock_hessian)
    if hessian_kind == "diag_quadratic":
        a, c, x0 = K.diag_quadratic_inputs(n, False)
        return Kernel(contexts, solver, amd.DiagQuadratic(a, c), x0, **mapping), lambda x: K.diag_quadratic_hessian(a)
    p, x0 = K.kappa_batch(n)
    objective = _dense_second(amd, p) if solver == "lbfgs" else _dense(amd, p)
    return Kernel(contexts, solver, objective, x0, user=True, **mapping), lambda x: K.dense_hessian(p, x)


# one problem per (kernel, Hessian, n, mapping) of parts 1 - 3.  Rosenbrock at n = 1 has H = (0) and no value (NaN): the
# DiagQuadratic problem stands in for it there.
RECORDED = [(s + "/rosenbrock", n, W, 1) for s in NEWTON for n, W in K.NEWTON_PAIRS if n > 1] + \
           [(s + "/diag_quadratic", 1, 8, 1) for s in NEWTON] + \
           [("lbfgs/rosenbrock", n, W, E) for n in K.ROSENBROCK_DIMS for W, E in _lbfgs_mappings(n)] + \
           [(s + "/dense", n, T.padded_width(n), 1) for s in NEWTON for n in K.DENSE_DIMS] + \
           [("lbfgs/dense", n, K.two_row_width(n), 2) for n in K.LBFGS_TWO_ROW_DIMS] + \
           [("lbfgs/dense", n, T.padded_width(n), 1) for n in K.LBFGS_ONE_ROW_DIMS]


@pytest.mark.parametrize("kind,n,W,E", RECORDED)
def test_device_value_by_bisection(contexts, kind, n, W, E):
    """Problem 0 of the batch: the threshold bisected between lo and hi down to two adjacent doubles, t and its
    successor, with the kernel stopping on t and not on the successor: the device's value is the successor, exactly.
    The assertion is the bracket (it stops on lo and not on hi); |c_dev - c_twin| / (c_twin u) is printed beside its bound
    2 n^2 + 8 for the table of DESIGN.md section 5."""
    kernel, hessian = _record_kernel(contexts, kind, n, W, E)
    iterates, values, _ = baseline(kernel, hessian, 1, "%s n = %d" % (kind, n))
    c = values[0][0]
    lo, hi = K.thresholds(c, n)

    def fires(t):
        x, status, iters = kernel.run(1, t)
        if status[0] == K.CONDITION:
            assert iters[0] == 1 and _same_rows(x[0], iterates[0][0])
            return True
        assert status[0] == K.ITERATION_LIMIT and iters[0] == 2
        return False

    assert fires(lo), "%s n = %d: the device's value is not above c (1 - delta), c = %r" % (kind, n, c)
    assert not fires(hi), "%s n = %d: the device's value is above c (1 + delta), c = %r" % (kind, n, c)
    a, b = np.array([lo, hi]).view(np.int64).tolist()        # positive doubles order as their bit patterns
    while b - a > 1:
        mid = (a + b) // 2
        if fires(float(np.array([mid], dtype=np.int64).view(np.float64)[0])):
            a = mid
        else:
            b = mid
    c_dev = float(np.array([b], dtype=np.int64).view(np.float64)[0])
    assert kernel.launches <= 64
    assert kernel.mapping == (W, E)
    print("\nCONDITION VALUE %s n = %d mapping %dx%d: twin %r device %r |c_dev - c_twin| / (c_twin u) = %.3g, bound %d"
          % (kind, n, W, E, c, c_dev, abs(c_dev - c) / (c * K.U), 2 * n * n + 8))
