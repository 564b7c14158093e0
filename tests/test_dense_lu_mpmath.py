"""The CPU twin's dense linear algebra (tests/newton_descent/nd_twin.hpp lu_factor / lu_solve / condition, and the
trust-region twin's own copy of condition) against elimination in high precision.  The device is held to the twin bit
for bit elsewhere; this file is what holds the twin to the mathematics.

Inputs: the recorded dense matrices H(x0) + safe_guard I of the Newton-descent golden file (every distinct one) and
RANDOM_PER_N seeded random dense matrices per n, n in dense_cases.DIMS.

Arithmetic.  The reference elimination runs in fixed point with FRACTION_BITS = 240 binary digits behind the point
(Python integers in numpy object arrays: 72 decimal digits of absolute resolution on entries of order 1 to 1e6, and the
only way to get through n = 64 a hundred times in the time a test may take — mpmath's own mpf needs 2 s per matrix
there).  mpmath at 50 digits runs where it is affordable: the residual b - A x of every solve is evaluated in mpmath from
the exact doubles, and at n <= 17 every matrix is also eliminated by an mpmath loop whose pivots and condition number the
fixed-point run must reproduce (test_fixed_point_elimination_is_mpmath_at_50_digits).

Checks.
  pivot order   the twin's pivot sequence is that of first-maximum partial pivoting in high precision.  A matrix on which
                the high-precision run meets two candidates within relative 2^-40 of each other is excluded — at most 2 %
                of the random ones; a recorded one only if the tie is exact, and an exact tie in the first column (whose
                entries are the inputs themselves) is not excluded at all: the first maximum has to win there.
  solve         |b - A x_hat| <= gamma_3n (P^T |L_hat| |U_hat|) |x_hat| componentwise, gamma_k = k u / (1 - k u),
                u = 2^-53: the backward-error theorem of Gaussian elimination, stated with the computed factors.  It has
                no free constant.
  condition     |cond_twin - cond| / cond <= CONDITION_C[n] n u cond.  The largest ratio |cond_twin - cond| / (n u cond^2)
                measured on these inputs falls with n, from 0.4707 at n = 2 (a random matrix; 0.1912 over the recorded
                ones) to 0.0025 at n = 64, so the bound is set per n: MEASURED_CONDITION_RATIO[n], and CONDITION_C[n]
                4 times that, for other seeds.  A matrix left out of the pivot comparison still goes through the solve
                and the condition check; no recorded matrix may be left out."""
import mpmath
import numpy as np
import pytest

import dense_cases as D
import nd_cases
import nd_lib as T

RANDOM_PER_N = 100
FRACTION_BITS = 240
ONE = 1 << FRACTION_BITS
U = 2.0 ** -53
MEASURED_CONDITION_RATIO = {2: 0.4707, 3: 0.1381, 7: 0.03029, 8: 0.04426, 9: 0.03936, 16: 0.01194, 17: 0.01139,
                            32: 0.006608, 33: 0.005829, 63: 0.00237, 64: 0.002525}
CONDITION_C = {n: 4 * r for n, r in MEASURED_CONDITION_RATIO.items()}


def to_fixed(a):
    """doubles -> exact fixed-point integers (object array of the same shape)"""
    flat = []
    for v in np.asarray(a, dtype=np.float64).reshape(-1).tolist():
        num, den = v.as_integer_ratio()             # den is a power of two
        assert ONE % den == 0, "a double below the fixed-point resolution"
        flat.append(num * (ONE // den))
    out = np.empty(len(flat), dtype=object)
    out[:] = flat
    return out.reshape(np.shape(a))


def to_mpf(v):
    return mpmath.mpf(int(v)) / ONE


class Elimination:
    """First-maximum partial-pivoting LU of A ([n, n] doubles) in fixed point: piv, near_tie (some column had two
    candidates within relative 2^-40 that were not equal), exact_tie_after_first (an exact tie in a column k > 0),
    inverse_norm2 (||A^-1||_F^2) and norm2 (||A||_F^2), both fixed point."""

    def __init__(self, A, want_inverse=True):
        n = A.shape[0]
        M = to_fixed(A)
        self.norm2 = int((M * M).sum()) >> FRACTION_BITS
        self.piv = np.zeros(n, dtype=np.int32)
        self.near_tie = self.exact_tie_after_first = False
        perm = list(range(n))
        for k in range(n):
            col = [abs(v) for v in M[k:, k]]
            best = max(col)
            p = col.index(best)                      # the first maximum
            for i, v in enumerate(col):
                if i != p and v == best:
                    self.exact_tie_after_first |= k > 0
                elif i != p and (best - v) * (1 << 40) <= best:
                    self.near_tie = True
            self.piv[k] = k + p
            if p:
                M[[k, k + p]] = M[[k + p, k]]
                perm[k], perm[k + p] = perm[k + p], perm[k]
            assert best != 0, "singular in high precision"
            if k + 1 < n:
                l = (M[k + 1:, k] << FRACTION_BITS) // M[k, k]
                M[k + 1:, k] = l
                M[k + 1:, k + 1:] -= (l[:, None] * M[k, k + 1:][None, :]) >> FRACTION_BITS
        self.lu, self.perm = M, perm
        if want_inverse:
            X = np.zeros((n, n), dtype=object)       # rows of P: A^-1 = U^-1 L^-1 P
            for i in range(n):
                X[i, perm[i]] = ONE
            for j in range(n):                       # unit lower triangle, column oriented
                if j + 1 < n:
                    X[j + 1:, :] -= (M[j + 1:, j][:, None] * X[j, :][None, :]) >> FRACTION_BITS
            for j in range(n - 1, -1, -1):           # upper triangle, last column first
                X[j, :] = (X[j, :] << FRACTION_BITS) // M[j, j]
                if j:
                    X[:j, :] -= (M[:j, j][:, None] * X[j, :][None, :]) >> FRACTION_BITS
            self.inverse_norm2 = int((X * X).sum()) >> FRACTION_BITS

    def condition(self):
        with mpmath.workdps(50):
            return mpmath.sqrt(to_mpf(self.norm2)) * mpmath.sqrt(to_mpf(self.inverse_norm2))


def recorded_matrices():
    """{n: [(name, A)]}: H(x0) + safe_guard I of every row of every dense case, each distinct matrix once"""
    out, seen = {}, set()
    for c in nd_cases.load_cases():
        if not c["name"].startswith("dense_"):
            continue
        n = c["x0"].shape[1]
        for r, x in enumerate(c["x0"]):
            A = D.hessian(c["params"], x)
            A[np.arange(n), np.arange(n)] = A[np.arange(n), np.arange(n)] + float(c["config"]["safe_guard"][0])
            if A.tobytes() not in seen:
                seen.add(A.tobytes())
                out.setdefault(n, []).append(("%s row %d" % (c["name"], r), A))
    return out


RECORDED = recorded_matrices()


def random_matrices(n):
    rng = np.random.default_rng([20261018, n])
    return [("random %d" % i, rng.standard_normal((n, n))) for i in range(RANDOM_PER_N)]


def check_matrix(name, A, rng, recorded):
    """-> (excluded, condition ratio); asserts the three properties"""
    n = A.shape[0]
    ref = Elimination(A)
    if ref.near_tie and recorded:
        raise AssertionError(name + ": a recorded matrix has a near (not exact) pivot tie")
    excluded = ref.near_tie or ref.exact_tie_after_first    # from the pivot comparison alone: the rest needs no unique pivot
    LU, piv = T.twin_lu(A)
    if not excluded:
        assert piv.tolist() == ref.piv.tolist(), "%s: pivots %s, high precision %s" % (name, piv.tolist(), ref.piv.tolist())
    # the solve: r = b - A x_hat in mpmath from the exact doubles; the bound from the twin's factors, in fixed point
    b = rng.standard_normal(n)
    x = T.twin_lu_solve(LU, piv, b)
    with mpmath.workdps(50):
        r = [abs(mpmath.mpf(float(b[i])) - mpmath.fdot(A[i].tolist(), x.tolist())) for i in range(n)]
        gamma = mpmath.mpf(3 * n) * mpmath.mpf(2) ** -53 / (1 - mpmath.mpf(3 * n) * mpmath.mpf(2) ** -53)
        L = to_fixed(np.abs(np.tril(LU, -1) + np.eye(n)))
        Uf = to_fixed(np.abs(np.triu(LU)))
        w = (Uf @ to_fixed(np.abs(x))) >> FRACTION_BITS
        w = (L @ w) >> FRACTION_BITS                      # |L||U||x| for the rows of P A
        rows = list(range(n))
        for k in range(n):
            rows[k], rows[piv[k]] = rows[piv[k]], rows[k]     # row k of P A is row rows[k] of A
        for k in range(n):
            bound = gamma * (to_mpf(w[k]) + mpmath.mpf(2) ** -200)    # (+ the fixed-point floor of the two products)
            assert r[rows[k]] <= bound, "%s: residual %s above the backward-error bound %s in row %d" % (
                name, mpmath.nstr(r[rows[k]], 5), mpmath.nstr(bound, 5), rows[k])
        cond = ref.condition()
        ratio = 0.0
        for twin_condition in (T.twin_condition, tr_twin_condition):
            err = abs(mpmath.mpf(twin_condition(A)) - cond) / cond
            ratio = max(ratio, float(err / (n * U * cond)))
    return excluded, ratio


_tr = []


def tr_twin_condition(A):
    """the trust-region twin's copy of the condition number (tests/trust_region/tr_twin.hpp)"""
    import ctypes as C
    import tr_lib
    if not _tr:
        fn = C.CDLL(tr_lib.TWIN_LIB).tr_twin_condition
        fn.restype, fn.argtypes = C.c_double, [C.c_void_p, C.c_int]
        _tr.append(fn)
    a = np.ascontiguousarray(np.asarray(A, dtype=np.float64).T).reshape(-1).copy()
    return _tr[0](a.ctypes.data, A.shape[0])


@pytest.mark.parametrize("n", D.DIMS)
def test_twin_lu_against_high_precision(n):
    rng = np.random.default_rng([20261019, n])
    assert len(RECORDED.get(n, [])) >= 8, "no recorded dense matrices at n = %d" % n
    worst = 0.0
    for name, A in RECORDED[n]:
        excluded, ratio = check_matrix(name, A, rng, recorded=True)
        assert not excluded, name + ": excluded from the pivot comparison (an exact tie past the first column)"
        worst = max(worst, ratio)
    print("n = %d: recorded matrices: largest |cond_twin - cond| / (n u cond^2) = %.4g" % (n, worst))
    excluded_random = 0
    for name, A in random_matrices(n):
        excluded, ratio = check_matrix("n = %d %s" % (n, name), A, rng, recorded=False)
        excluded_random += excluded
        worst = max(worst, ratio)
    assert excluded_random <= 0.02 * RANDOM_PER_N, "%d random matrices excluded for near ties" % excluded_random
    print("n = %d: largest |cond_twin - cond| / (n u cond^2) = %.4g" % (n, worst))
    assert worst <= CONDITION_C[n], "condition number off by %.4g n u cond (bound %.4g)" % (worst, CONDITION_C[n])


def test_recorded_matrices_hold_exact_first_column_ties():
    """Some recorded matrix at n >= 9 has its first column's maximum twice: the twin takes the first (checked above
    against the high-precision pivots, which take the first by construction)."""
    found = 0
    for n, items in RECORDED.items():
        for name, A in items:
            col = np.abs(A[:, 0])
            found += n >= 9 and int((col == col.max()).sum()) > 1
    assert found >= 1


@pytest.mark.parametrize("n", [m for m in D.DIMS if m <= 17])
def test_fixed_point_elimination_is_mpmath_at_50_digits(n):
    """The arithmetic of the reference itself: an mpmath loop at 50 digits gives the pivots of the fixed-point run and its
    condition number to 40 digits, on the first recorded matrices and the first random ones of this n."""
    for name, A in RECORDED[n][:4] + random_matrices(n)[:6]:
        ref = Elimination(A)
        if ref.near_tie or ref.exact_tie_after_first:
            continue
        with mpmath.workdps(50):
            M = mpmath.matrix(A.tolist())
            piv = []
            for k in range(n):
                col = [abs(M[i, k]) for i in range(k, n)]
                p = k + col.index(max(col))
                piv.append(p)
                if p != k:
                    for j in range(n):
                        M[k, j], M[p, j] = M[p, j], M[k, j]
                for i in range(k + 1, n):
                    M[i, k] = M[i, k] / M[k, k]
                    for j in range(k + 1, n):
                        M[i, j] = M[i, j] - M[i, k] * M[k, j]
            assert piv == ref.piv.tolist(), name
            Am = mpmath.matrix(A.tolist())
            cond = mpmath.mnorm(Am, "f") * mpmath.mnorm(mpmath.inverse(Am), "f")
            assert abs(cond - ref.condition()) <= mpmath.mpf(10) ** -40 * cond, name
