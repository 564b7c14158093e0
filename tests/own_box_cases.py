"""Inputs of the per-problem-bounds tests (BatchedLbfgsb.SetBoundsPerProblem, mi355_lbfgsb_minimize_batch_boxes).

Seven cases — the smallest shapes that reach every kernel path built for one box per problem — of B = 131 problems
each.  Row b takes box b mod 9 of the nine boxes below; 9 is coprime to the four segments of a wavefront, so neighbouring
segments, and consecutive fetches of one segment under a capped grid, always hold different boxes.

The twin of a case is put together from the oracles as they are (one box per call): one call per box, on that box's rows.
It is computed once per (case, stopping preset) and shared by the tests of both modules.
"""
import numpy as np

B = 131
K = 9
DMAX = 1.7976931348623157e308
SEED = 20261019

# kernel: "exact" (lbfgsb_solve_kernel, twin oracle.lbfgsb_minimize_batch with the butterfly order at width 16 E) or
# "relaxed" (lbfgsb_fast_kernel, twin oracle.lbfgsb_fast_minimize_batch)
CASES = [
    dict(name="exact_n5_m3", kernel="exact", n=5, m=3, objective="rosenbrock"),           # E = 1, padding lanes
    dict(name="exact_n32_m5", kernel="exact", n=32, m=5, objective="rosenbrock"),         # E = 2, no padding
    dict(name="exact_n40_m7", kernel="exact", n=40, m=7, objective="rosenbrock"),         # E = 4, capacity 8
    dict(name="exact_ridge_n8_m5", kernel="exact", n=8, m=5, objective="squared_error_ridge", rows=12),
    dict(name="relaxed_n5_m3", kernel="relaxed", n=5, m=3, objective="rosenbrock"),       # E = 1
    dict(name="relaxed_n32_m5", kernel="relaxed", n=32, m=5, objective="rosenbrock"),     # E = 2
    dict(name="relaxed_n20_m7", kernel="relaxed", n=20, m=7, objective="rosenbrock"),     # E = 2, capacity 8
]
BY_NAME = {c["name"]: c for c in CASES}
EXACT = [c["name"] for c in CASES if c["kernel"] == "exact"]
RIDGE_LAMBDA = 0.05


def boxes(n):
    """The nine boxes as (lower [9, n], upper [9, n])."""
    j = np.arange(n)
    lo, hi = np.empty((K, n)), np.empty((K, n))
    lo[0], hi[0] = -DMAX, DMAX                      # 1 the default box
    lo[1], hi[1] = -1.5, 0.8                        # 2 the Rosenbrock minimiser (all ones) lies outside
    lo[2], hi[2] = -3.0, 3.0                        # 3 ... inside
    lo[3], hi[3] = -DMAX, 0.5                       # 4 one-sided
    lo[4], hi[4] = -2.0, 2.0                        # 5 every third coordinate fixed
    lo[4, ::3] = hi[4, ::3] = 0.7
    lo[5], hi[5] = 0.9, 0.95                        # 6 a corner box
    lo[6], hi[6] = -1.5 + 0.03 * j, 0.6 + 0.04 * j  # 7 another interval on each coordinate
    lo[7], hi[7] = 2.5, 3.5                         # 8 every start (in [-2, 2]) violates it on every coordinate
    lo[8], hi[8] = -1.0, 1.25                       # 9 the start lies on the lower / upper bound in half the coordinates
    return lo, hi


def box_of_row():
    return np.arange(B) % K


def inputs(case):
    """x0 [B, n], lower [B, n], upper [B, n], per-problem data (or None) of a case; fresh arrays on every call."""
    import cppnumericalsolvers_amd as amd
    n = case["n"]
    x0 = amd.synthetic_x0_host(B, n, "u2", seed=SEED + 100 * n + case["m"])
    assert np.abs(x0).max() <= 2.0
    blo, bhi = boxes(n)
    which = box_of_row()
    lower, upper = blo[which].copy(), bhi[which].copy()
    on = which == 8                                 # box 9: coordinates 0, 4, 8, .. start on the lower bound, 2, 6, .. on the upper
    x0[np.ix_(on, np.arange(0, n, 4))] = -1.0
    x0[np.ix_(on, np.arange(2, n, 4))] = 1.25
    violates = (x0[which == 7] < 2.5).all()
    assert violates
    per_problem = None
    if case["objective"] == "squared_error_ridge":
        per_problem = np.random.default_rng(SEED + 7).normal(size=(B, case["rows"])) * 3.0
    return x0, lower, upper, per_problem


def inputs_digest(x0, lower, upper):
    """SHA-256 of the inputs of a case (what tests/golden/own_box_reference_n40_m7.npz was recorded for)."""
    import hashlib
    h = hashlib.sha256()
    for a in (x0, lower, upper):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def recorded_reference(name):
    """(x, f) of the reference's Lbfgsb on a case whose history size the reference binary does not hold
    (tests/golden/make_golden_own_box.py), or None."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "own_box_reference_%s.npz" % name[len("exact_"):])
    if not os.path.exists(path):
        return None
    z = np.load(path)
    assert str(z["inputs_sha256"]) == inputs_digest(*inputs(BY_NAME[name])[:3]), "the recorded reference is of other inputs"
    return z["x"], z["f"]


def ridge_matrix(case):
    return np.random.default_rng(SEED + 11).normal(size=(case["rows"], case["n"]))


def engine_objective(case):
    import cppnumericalsolvers_amd as amd
    if case["objective"] == "squared_error_ridge":
        return amd.SquaredErrorRidge(ridge_matrix(case), RIDGE_LAMBDA)
    return amd.Rosenbrock()


def exact_width(n):
    """Padded width 16 E of the reference-order kernel's mapping (what the butterfly order of the twin follows)."""
    return 16 * (1 if n <= 16 else (2 if n <= 32 else 4))


def stop_of(oracle, preset):
    return {"default": oracle.lbfgsb_default_stop, "parity": oracle.parity_stop}[preset]()


def twin_rows(oracle, case, stop, x0, lower, upper, per_problem):
    """The oracle of the case's kernel on rows that all have ONE box (lower / upper: n doubles)."""
    kw = dict(m=case["m"], stop=stop, lower=lower, upper=upper, per_problem=per_problem)
    if case["objective"] == "squared_error_ridge":
        kw["params"] = oracle.ridge_params(ridge_matrix(case), RIDGE_LAMBDA)
    if case["kernel"] == "exact":
        return oracle.lbfgsb_minimize_batch(case["objective"], x0, reduction="butterfly", width=exact_width(case["n"]), **kw)
    return oracle.lbfgsb_fast_minimize_batch(case["objective"], x0, **kw)


_twins = {}


def twin(oracle, name, preset):
    """(x, f, g, progress) of the whole batch of a case: nine oracle calls, one per box, on that box's rows.  Cached;
    callers must not write to it."""
    key = (name, preset)
    if key not in _twins:
        case = BY_NAME[name]
        x0, lower, upper, pp = inputs(case)
        blo, bhi = boxes(case["n"])
        which = box_of_row()
        out = None
        for k in range(K):
            rows = np.flatnonzero(which == k)
            assert (lower[rows] == blo[k]).all() and (upper[rows] == bhi[k]).all()
            part = twin_rows(oracle, case, stop_of(oracle, preset), x0[rows], blo[k], bhi[k], None if pp is None else pp[rows])
            if out is None:
                out = tuple(np.zeros((B,) + a.shape[1:], dtype=a.dtype) for a in part)
            for dst, src in zip(out, part):
                dst[rows] = src
        for a in out:
            a.setflags(write=False)
        _twins[key] = out
    return _twins[key]


def same_bits(got, want, what, fields=None):
    """x, f, g and every progress field, bit for bit."""
    for name, a, b in zip(("x", "f", "g"), got[:3], want[:3]):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        bad = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs in rows %s" % (what, name, bad[:8])
    for k in fields or want[3].dtype.names:
        same = np.ascontiguousarray(got[3][k]).tobytes() == np.ascontiguousarray(want[3][k]).tobytes()
        assert same, "%s: progress.%s differs in rows %s" % (what, k, np.flatnonzero(got[3][k] != want[3][k])[:8])
