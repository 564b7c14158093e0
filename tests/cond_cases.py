"""Inputs and host arithmetic of the condition-number brackets (tests/test_cond_bracket_cpu.py on the CPU,
tests/test_gpu_condition_value.py on the device).

The solve kernels compute ||H||_F ||H^-1||_F of every iterate in LDS (csrc/hessian_condition_device.hpp) and report one
bit of it: `condition > stop.condition_hessian` (status 5).  The tests here pin the VALUE: for an iterate x the host
builds H(x) in the functor's own operation order (bit for bit what hess_full writes), takes the CPU twin's condition
number c of it, and launches the kernel with the thresholds

    lo = c (1 - delta) rounded down,    hi = c (1 + delta) rounded up,    delta = (2 n^2 + 8) u,  u = 2^-53:

the device must stop on lo and must not stop on hi.

delta is derived.  The kernel's LU and substitutions do the twin's element operations (that claim of the kernel's header
is what these tests check), so device and twin differ in the ORDER of two sums of N = n^2 non-negative squares — any order
of such a sum is within (N - 1) u of the exact sum, relative — two square roots (their arguments' errors are halved, their
own rounding is u each), one product (u) and the two roundings of the thresholds: (2 n^2 + 8) u covers all of it to first
order with room to spare at every n (9.1e-13 at n = 64, 1.8e-15 at n = 2).

condition() below is a numpy/Python copy of the twin's `condition` (tests/newton_descent/nd_twin.hpp: the same element
operations in the same order, bit for bit — asserted by tests/test_cond_bracket_cpu.py) into which the deliberate bugs of
MUTATIONS can be planted: what a wrong kernel would compute, against the same brackets."""
import math

import numpy as np

import dense_cases as D

U = 2.0 ** -53
ITERATION_LIMIT, CONDITION = 1, 5      # MI355_STATUS_ITERATION_LIMIT, MI355_STATUS_HESSIAN_CONDITION_VIOLATION
B = 8                                  # problems per case
MAX_CONDITION = 1e15                   # every bracketed condition number is finite and below this

# ---- the bracket -------------------------------------------------------------------------------------------------------


def delta(n):
    return (2 * n * n + 8) * U


def thresholds(c, n):
    """(lo, hi): c (1 - delta) rounded down and c (1 + delta) rounded up (one step past the rounded-to-nearest product)"""
    d = delta(n)
    return float(np.nextafter(c * (1.0 - d), -np.inf)), float(np.nextafter(c * (1.0 + d), np.inf))


def inside(value, c, n):
    """Whether a kernel that computed `value` would pass the bracket of c: stop on lo (value > lo), not on hi."""
    lo, hi = thresholds(c, n)
    return bool(value > lo) and not bool(value > hi)


def clear_of(c, t, n):
    """|c - t| > delta t: the decision c > t is the device's too (used for the other problems of a launch)"""
    return abs(c - t) > delta(n) * t


def separated(cs, n):
    """no two of the condition numbers within 4 delta of each other (relative to the larger)"""
    s = np.sort(np.asarray(cs, dtype=np.float64))
    return bool(np.all(np.diff(s) > 4 * delta(n) * s[1:]))


# ---- host Hessians, in the functors' operation order -------------------------------------------------------------------


def rosenbrock_hessian(x):
    """csrc/objectives.hpp hess_diag / RosenbrockConditionObjective::hess_full: H[i, j] = H(i, j)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    H = np.zeros((n, n))
    for j in range(n):
        has_a, has_b = j + 1 < n, j > 0
        a = (((1200.0 * x[j]) * x[j] - 400.0 * x[j + 1]) + 2.0) if has_a else 0.0
        H[j, j] = (a + 200.0) if (has_a and has_b) else (a if has_a else (200.0 if has_b else 0.0))
        if has_a:
            H[j + 1, j] = H[j, j + 1] = -400.0 * x[j]
    return H


def diag_quadratic_hessian(a):
    """DiagQuadraticHessObjective::hess_full: diag(2 a)"""
    return np.diag(2.0 * np.asarray(a, dtype=np.float64))


def dense_hessian(params, x):
    """examples/user_objective_dense/dense_quartic.hpp hess_full: S(i, i) + (3 kappa)(x_i x_i) on the diagonal"""
    return D.hessian(np.asarray(params, dtype=np.float64), np.asarray(x, dtype=np.float64))


def dense_params(S, b, kappa):
    """the functor's parameter block: S column major, b, kappa"""
    return np.concatenate([np.asarray(S, dtype=np.float64).T.reshape(-1), np.asarray(b, dtype=np.float64), [float(kappa)]])


# ---- the twin's condition number in numpy, with deliberate bugs --------------------------------------------------------

NO_MUTATION = None
LAST_INVERSE_COLUMN_DROPPED = "the last column of the inverse left out of its norm"
SECOND_ROW_NOT_UPDATED = "a lane's second row of the trailing block (rows k + 1 + sl + W) not updated"
PIVOT_LAST_MAXIMUM = "the pivot taken as the last maximum of the column, not the first"
BUTTERFLY_LEVEL_DROPPED = "the first butterfly level of the ||H|| sum dropped (the odd lanes' partial sums missing)"
INTERCHANGES_SKIPPED = "the row interchanges of the unit vector skipped"
MUTATIONS = (LAST_INVERSE_COLUMN_DROPPED, SECOND_ROW_NOT_UPDATED, PIVOT_LAST_MAXIMUM, BUTTERFLY_LEVEL_DROPPED,
             INTERCHANGES_SKIPPED)


def two_row_width(n):
    """lanes per problem of the Lbfgs mapping with two coordinates per lane that holds n (8, 16 or 32)"""
    W = 8
    while 2 * W < n:
        W *= 2
    return W


class Factorisation:
    """The twin's lu_factor on A[i, j] = A(i, j): lu, piv, and what the pivot searches met."""

    def __init__(self, A, mutation=NO_MUTATION, W=8):
        a = np.array(A, dtype=np.float64)
        n = a.shape[0]
        self.piv, self.ties, self.first_column_ties, self.max_pivot_distance, self.zero_columns = [], 0, 0, 0, 0
        with np.errstate(all="ignore"):
            for k in range(n):
                col = np.abs(a[:, k]).tolist()
                p, best = k, col[k]
                for i in range(k + 1, n):
                    if col[i] > best or (mutation == PIVOT_LAST_MAXIMUM and col[i] == best):
                        p, best = i, col[i]
                self.piv.append(p)
                tied = best != 0.0 and sum(v == best for v in col[k:]) > 1
                self.ties += tied
                self.first_column_ties += tied and k == 0
                self.zero_columns += best == 0.0
                self.max_pivot_distance = max(self.max_pivot_distance, self.piv[k] - k)
                if best != 0.0:
                    if p != k:
                        a[[k, p], :] = a[[p, k], :]
                    a[k + 1:, k] = a[k + 1:, k] / a[k, k]
                new = a[k + 1:, k + 1:] - a[k + 1:, k][:, None] * a[k, k + 1:][None, :]
                if mutation == SECOND_ROW_NOT_UPDATED:
                    new[W:2 * W, :] = a[k + 1:, k + 1:][W:2 * W, :]
                a[k + 1:, k + 1:] = new
        self.lu = a


def condition(A, mutation=NO_MUTATION, W=8):
    """nd_twin.hpp `condition` element operation by element operation (W: the lanes per problem a lane-wise mutation
    refers to)."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    sh = 0.0
    for t, v in enumerate(A.T.reshape(-1).tolist()):          # the chain over the column-major storage
        if mutation == BUTTERFLY_LEVEL_DROPPED and (t % W) & 1:
            continue
        sh += v * v
    F = Factorisation(A, mutation, W)
    a = F.lu
    X = np.eye(n)                                             # column c: the unit vector e_c
    with np.errstate(all="ignore"):
        if mutation != INTERCHANGES_SKIPPED:
            for k in range(n):
                if F.piv[k] != k:
                    X[[k, F.piv[k]], :] = X[[F.piv[k], k], :]
        for j in range(n):
            X[j + 1:, :] = X[j + 1:, :] - X[j, :][None, :] * a[j + 1:, j][:, None]
        for j in range(n - 1, -1, -1):
            X[j, :] = X[j, :] / a[j, j]
            X[:j, :] = X[:j, :] - X[j, :][None, :] * a[:j, j][:, None]
    si = 0.0
    columns = n - 1 if mutation == LAST_INVERSE_COLUMN_DROPPED else n
    for v in X.T.reshape(-1).tolist()[:columns * n]:          # column after column, each ascending
        si += v * v
    return math.sqrt(sh) * math.sqrt(si)


# ---- the dense matrices (H = S with kappa = 0) -------------------------------------------------------------------------

DENSE_DIMS = (2, 7, 8, 9, 17, 33, 64)              # under NewtonDescent and TrustRegionNewton
LBFGS_TWO_ROW_DIMS = (9, 16, 17, 33, 63, 64)       # under Lbfgs with two coordinates per lane
LBFGS_ONE_ROW_DIMS = (8, 33, 64)                   # ... with one
ALL_DENSE_DIMS = tuple(sorted(set(DENSE_DIMS + LBFGS_TWO_ROW_DIMS + LBFGS_ONE_ROW_DIMS)))
RANDOM_CONDITIONS = (1e1, 1e4, 1e8, 1e12)
SINGULAR = "zero first column"


def _recorded(n):
    """[(name, H(x0) + safe_guard I)] of the Newton-descent golden file's dense cases at this n: the matrices whose LU
    was recorded against the reference (tests/golden/make_golden_nd.py), each distinct one once"""
    import nd_cases
    out, seen = [], set()
    for c in nd_cases.load_cases():
        if not c["name"].startswith("dense_") or c["x0"].shape[1] != n:
            continue
        for r, x in enumerate(c["x0"]):
            A = D.hessian(c["params"], x)
            A[np.arange(n), np.arange(n)] = A[np.arange(n), np.arange(n)] + float(c["config"]["safe_guard"][0])
            if A.tobytes() not in seen:
                seen.add(A.tobytes())
                out.append(("%s row %d" % (c["name"], r), A))
    return out


def random_matrix(n, cond, seed):
    """orthogonal x diag(singular values from 1 down to 1 / cond, log spaced) x orthogonal"""
    rng = np.random.default_rng([20261020, n, seed])
    Q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0.0, -math.log10(cond), n)
    return (Q1 * s[None, :]) @ Q2.T


_matrices = {}


def dense_matrices(n):
    """[(name, S)] at this n.  From the recorded matrices (n of dense_cases.DIMS): the SPD one whose pivots lie farthest
    from the diagonal, one with an exact tie in its first column where there is one, the most interchanges (fill-in:
    the SPD family's S = diag(2^k) C diag(2^k) is dense), the asymmetric (1 + 2^-50) variant; the indefinite family's S;
    random matrices with the condition numbers of RANDOM_CONDITIONS, those of 1e8 and 1e12 a second time with an exact
    tie planted in the first column; last the singular one (SINGULAR)."""
    if n in _matrices:
        return _matrices[n]
    out = []
    recorded = _recorded(n) if n in D.DIMS else []
    stats = [(name, A, Factorisation(A)) for name, A in recorded]
    spd = [s for s in stats if "_spd_" in s[0]]
    if spd:
        far = max(spd, key=lambda s: s[2].max_pivot_distance)
        out.append(("far pivots: " + far[0], far[1]))
        tie = [s for s in spd if s[2].first_column_ties and s[0] != far[0]]
        if tie:
            out.append(("first-column tie: " + tie[0][0], tie[0][1]))
        most = max(spd, key=lambda s: sum(p != k for k, p in enumerate(s[2].piv)))
        if most[0] not in (far[0], tie[0][0] if tie else None):
            out.append(("most interchanges: " + most[0], most[1]))
    asym = [s for s in stats if "_asym_" in s[0]]
    if asym:
        out.append(("asymmetric: " + asym[0][0], asym[0][1]))
    out.append(("indefinite family", D.matrix(D.integers(3, n, indefinite=True))))
    for i, cond in enumerate(RANDOM_CONDITIONS):
        A = random_matrix(n, cond, i)
        out.append(("random, condition %.0e" % cond, A))
        if cond >= 1e8:
            # an exact tie in the first column, the second candidate in the middle row (or the one before): the first
            # maximum and the last are then different factorisations of an ill-conditioned matrix
            T = A.copy()
            p = int(np.argmax(np.abs(T[:, 0])))
            T[n // 2 if p != n // 2 else n // 2 - 1, 0] = -T[p, 0]
            out.append(("random with a first-column tie, condition %.0e" % cond, T))
    out.append((SINGULAR, D.matrix(D.integers(7, n, flags=D.ZERO_FIRST))))
    _matrices[n] = out
    return out


def dense_starts(n, seed=0):
    """B starts of the dense functor: multiples of 1 / 128 in [-2, 2], as dense_cases.starts"""
    return np.random.default_rng([20261021, n, seed]).integers(-256, 257, (B, n)).astype(np.float64) / 128.0


def dense_rhs(n):
    return np.random.default_rng([20261022, n]).integers(-64, 65, n).astype(np.float64) / 64.0


def kappa_batch(n):
    """(params, x0) of the batch with kappa > 0: H(x) = S + 3 kappa diag(x^2) differs from problem to problem"""
    ints = D.integers(11, n, rows=B, kappa=0.5)
    return D.params(ints), D.starts(ints)


# ---- Rosenbrock and DiagQuadratic inputs -------------------------------------------------------------------------------

ROSENBROCK_DIMS = (2, 7, 8, 9, 16, 17, 32, 33, 63, 64)
# (n, lanes per problem) of tests/test_gpu_work_queue.py: every padded width with its boundaries, then the over-wide ones
NEWTON_PAIRS = ((1, 8), (7, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (63, 64), (64, 64), (7, 64),
                (12, 32))


def rosenbrock_starts(n):
    """(-1.2, 1) tiled; four rows uniform in [-2, 2]; three rows 1 + 1e-3 N(0, 1): next to the minimiser, where H is
    conditioned best and the brackets are narrowest in absolute terms"""
    rng = np.random.default_rng([20261023, n])
    return np.vstack([np.tile([-1.2, 1.0], n)[:n][None, :], rng.uniform(-2.0, 2.0, (4, n)),
                      1.0 + 1e-3 * rng.standard_normal((3, n))])


def diag_quadratic_inputs(n, indefinite):
    """(a, c, x0): coefficients of magnitude 2^-2 .. 2^3 times [1, 2); the indefinite model has every third one negative"""
    rng = np.random.default_rng([20261024, n, int(indefinite)])
    a = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-2, 4, n).astype(np.int32))
    if n == 1:
        a = np.array([2.0])              # H = (4): |4| fl(1 / 4) is 1 exactly
    if indefinite:
        a[::3] = -a[::3]
    return a, 0.25, rng.uniform(-2.0, 2.0, (B, n))


# The bracket at iterate 3: Rosenbrock n = 17, the first five starts (the rows next to the minimiser arrive at it, and at
# one Hessian, by iterate 3), and per solver the rows whose condition number at iterate 3 exceeds those at iterates 1 and
# 2 — a threshold at the value of iterate 3 lets the solve get there (Lbfgs: m = 5, exact, 16 lanes x 2 coordinates).
LATER_ITERATE_N = 17
LATER_ITERATE_ROWS = {"newton_descent": (1, 2, 3), "trust_region": (4,), "lbfgs": (1, 4)}


def later_iterate_starts():
    return rosenbrock_starts(LATER_ITERATE_N)[:5]
