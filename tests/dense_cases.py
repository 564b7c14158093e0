"""Inputs of the dense-Hessian functor (examples/user_objective_dense/dense_quartic.hpp, objective id 101) for the
Newton-descent and trust-region tests:  f(x) = 0.5 x.(S x) - b.x + (kappa / 4) sum x_i^4.

Everything is built from small integers with exact operations, so the same bytes come out on any machine, and the golden
files store the integers (`dense_M`, `dense_N`, `dense_k`, `dense_bq`, `dense_kappa`, `dense_flags`, `x0_q`) with a
SHA-256 of the rebuilt parameter block, checked on load:
    C = (M^T M - N^T N) / 4 + I / 8     M, N integer matrices with entries in [-2, 2] (N empty: the SPD family;
                                        N present: the indefinite family, without the I / 8)
    S = diag(2^k) C diag(2^k)           integer k_i in [-3, 3]: every entry an exact dyadic, S == S.T bitwise
    b = bq / 64,   x0 = x0_q / 128      |x0_q| <= 256 (int16)
Flags: ASYMMETRIC multiplies the strict upper triangle of S by 1 + 2^-50 (one correctly rounded product per entry): the
gradient moves by parts in 1e-15, H stops being bitwise symmetric, and reading H(j, i) for H(i, j) changes the bytes of
a solve.  ZERO_FIRST clears row and column 0 of S (S e_0 = 0): with kappa = 0 and safe_guard = 0 the LU's first column
has no non-zero entry.
The parameter block is S (n x n, column major), b (n), kappa: n n + n + 1 doubles.

Size: x* is recorded in full up to n = 33 and as a SHA-256 digest above it, g* as a digest throughout (the scheme of
fo_cases.py); f* and the progress fields are recorded in full.  A digest serves the bit-for-bit comparison as the bytes
do; where a test needs the reference's x* as numbers it takes the twin in reference order after checking its digest."""
import hashlib

import numpy as np

import fo_cases

DENSE = 101
DIMS = (2, 3, 7, 8, 9, 16, 17, 32, 33, 63, 64)
FULL_RECORD_MAX_N = 33
ASYMMETRIC, ZERO_FIRST = 1, 2
PREFIX = "dense_"            # the dense cases' members of a golden file: fo_cases.pack() of their arrays
INTEGER_KEYS = ("dense_M", "dense_N", "dense_k", "dense_bq", "dense_kappa", "dense_flags", "x0_q")


def integers(seed, n, indefinite=False, rows=8, kappa=1.0, flags=0, q_max=256):
    """The integers of one case, drawn from (seed, n)."""
    rng = np.random.default_rng([seed, n])
    m = n // 2 + 1
    M = rng.integers(-2, 3, (m, n)).astype(np.int8)
    N = rng.integers(-2, 3, (m, n)).astype(np.int8) if indefinite else np.zeros((0, n), dtype=np.int8)
    return dict(dense_M=M, dense_N=N, dense_k=rng.integers(-3, 4, n).astype(np.int8),
                dense_bq=rng.integers(-64, 65, n).astype(np.int16), dense_kappa=np.float64(kappa),
                dense_flags=np.int32(flags), x0_q=rng.integers(-q_max, q_max + 1, (rows, n)).astype(np.int16))


def matrix(ints):
    """S as an [n, n] array, S[i, j] = S(i, j)."""
    M, N, k = (ints[key].astype(np.int64) for key in ("dense_M", "dense_N", "dense_k"))
    n = M.shape[1]
    flags = int(ints["dense_flags"])
    c8 = 2 * (M.T @ M - N.T @ N) + (0 if N.shape[0] else 1) * np.eye(n, dtype=np.int64)      # 8 C, in integers
    S = np.ldexp(c8.astype(np.float64), (k[:, None] + k[None, :] - 3).astype(np.int32))
    assert S.tobytes() == np.ascontiguousarray(S.T).tobytes()
    if flags & ZERO_FIRST:
        S[0, :] = 0.0
        S[:, 0] = 0.0
    if flags & ASYMMETRIC:
        S = np.where(np.triu(np.ones((n, n), dtype=bool), 1), S * (1.0 + 2.0 ** -50), S)
    return S


def params(ints):
    """The functor's parameter block: S column major, b, kappa."""
    S = matrix(ints)
    return np.concatenate([S.T.reshape(-1), ints["dense_bq"].astype(np.float64) / 64.0, [float(ints["dense_kappa"])]])


def starts(ints):
    return ints["x0_q"].astype(np.float64) / 128.0


def hessian(p, x):
    """H(x) as an [n, n] array (row i, column j), with the functor's operations."""
    n = x.shape[0]
    H = p[:n * n].reshape(n, n).T.copy()
    H[np.arange(n), np.arange(n)] = H[np.arange(n), np.arange(n)] + (3.0 * p[n * n + n]) * (x * x)
    return H


def sha256(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


def record_results(rec, x, g):
    """x* and g* of the reference as the file keeps them (see the head of this module)."""
    if x.shape[1] <= FULL_RECORD_MAX_N:
        rec["x"] = x
    else:
        rec["x_sha256"] = sha256(x)
    rec["g_sha256"] = sha256(g)


def same_as_recorded(case, key, a):
    """a (x or g of a solve) against the reference's recorded bytes, or their digest"""
    if key in case:
        return a.tobytes() == case[key].tobytes()
    return sha256(a).tobytes() == case[key + "_sha256"].tobytes()


def reference_x(case, twin_x):
    """The reference's x*: recorded, or — digest cases — the reference-order twin's, which must have the recorded digest"""
    if "x" in case:
        return case["x"]
    assert same_as_recorded(case, "x", twin_x), case["name"] + ": the twin in reference order is not the recorded x"
    return twin_x


def pack(arrays):
    """{"case/key": array} of the dense cases -> the members they add to a golden file"""
    return {PREFIX + k: v for k, v in fo_cases.pack(arrays).items()}


def load(z, struct_dtypes):
    """The dense cases of an opened golden file, parameters and starts rebuilt and checked against the recorded hash."""
    if PREFIX + "index" not in z.files:
        return []
    arrays = fo_cases.unpack({k[len(PREFIX):]: z[k] for k in z.files if k.startswith(PREFIX)}, struct_dtypes)
    names = sorted({k.split("/")[0] for k in arrays})
    cases = [dict(name=nm, **{k.split("/")[1]: v for k, v in arrays.items() if k.split("/")[0] == nm}) for nm in names]
    for c in cases:
        c["params"] = params(c)
        assert sha256(c["params"]).tobytes() == c["params_sha256"].tobytes(), c["name"] + ": parameters rebuilt differently"
        c["x0"] = starts(c)
    return cases


def zero_column_case():
    """S e_0 = 0 with kappa = 0 and safe_guard = 0: the first column of the Newton-descent LU has no non-zero entry, so
    the factorisation takes its `best == 0` branch (no interchange, no division) and the solve divides by lu(0, 0) = 0.
    The reference's safe_guard is a compile-time 1e-5, so this case exists for the device against its twin only, capped
    at 3 iterations; the iterates are infinite or NaN from the first step on."""
    import nd_lib
    ints = integers(7, 9, rows=3, kappa=0.0, flags=ZERO_FIRST)
    return dict(name="dense_zero_column_n09", objective=np.int32(DENSE), params=params(ints), x0=starts(ints),
                stop=nd_lib.make_stop(**{**nd_lib.STOP_PRESETS["default"], "num_iterations": 3}),
                config=nd_lib.make_config(safe_guard=0.0), condition_stop=np.float64(0.0))


# (seed, binary exponent of the antisymmetric part) of chain_case(n)
CHAIN_CASES = {9: (2, 70), 17: (1, 60)}


def chain_case(n):
    """S = S_spd + 2^e K with K antisymmetric, small integers in its strict upper triangle (one correctly rounded sum per
    entry; the diagonal stays).  The Armijo search reads H only through v . d with v_j = sum_i (k d_i) H(i, j), and
    d'H d = d'H^T d, so walking row j for column j moves the bound by rounding alone: on every other case here that is a
    part in 1e16 and no trial notices.  With entries of 2^60 and more against a symmetric part of order 1, g = S x - b is
    of that size too, the Newton step d is of order 1, and the terms of v . d and of x . (S x) cancel down to their
    rounding: the bound and the trial values are of the size of that rounding, and the other walk takes another step
    length.  Nothing converges here (and the reference is not asked): the device against its twin only, three
    iterations, searches of up to some hundred trials."""
    import nd_lib
    seed, exponent = CHAIN_CASES[n]
    ints = integers(seed, n, rows=4)
    K = np.triu(np.random.default_rng([seed, n, 1]).integers(-2, 3, (n, n)), 1).astype(np.float64)
    S = matrix(ints) + np.ldexp(K - K.T, exponent)
    p = np.concatenate([S.T.reshape(-1), ints["dense_bq"].astype(np.float64) / 64.0, [1.0]])
    return dict(name="dense_chain_n%02d" % n, objective=np.int32(DENSE), params=p, x0=starts(ints),
                stop=nd_lib.make_stop(**{**nd_lib.STOP_PRESETS["default"], "num_iterations": 3}),
                config=nd_lib.make_config(), condition_stop=np.float64(0.0))


def nd_mutation_shows(mutation, case, orders=(0, 1)):
    """Whether the Newton-descent twin with a planted bug (nd_lib.TRANSPOSE_BEFORE_LU: H transposed before the LU;
    nd_lib.CHAIN_WALKS_ROW: the search's chain walking row j of H for column j) gives other bytes (x, f, g or a progress
    field) on at least one row of the case, in both summation orders."""
    import nd_lib
    args = (DENSE, case["x0"], case["params"], case["stop"], case["config"], float(case["condition_stop"]))
    for order in orders:
        good = nd_lib.twin_solve(*args, order=order)
        bad = nd_lib.twin_solve_mutated(mutation, *args, order=order)
        if all(good[k].tobytes() == bad[k].tobytes() for k in range(4)):
            return False
    return True


def nd_transposition_shows(case, orders=(0, 1)):
    """H transposed before the LU changes the bytes of the case.  (The 2^-50 of the ASYMMETRIC flag does not reach the
    chain of the search: chain_case.)"""
    import nd_lib
    return nd_mutation_shows(nd_lib.TRANSPOSE_BEFORE_LU, case, orders)


def tr_transposition_shows(case, orders=(0, 1)):
    """Whether the trust-region twin with H d walking a column of H for a row gives other bytes (x, f, g or a progress
    field) on at least one row of the case, in both summation orders."""
    import tr_lib
    args = (DENSE, case["x0"], case["params"], case["stop"], case["config"], float(case["condition_stop"]))
    for order in orders:
        good = tr_lib.twin_solve_ex(*args, order=order)
        bad = tr_lib.twin_solve_ex(*args, order=order, mutation=tr_lib.PRODUCT_WALKS_COLUMN)
        if all(good[k].tobytes() == bad[k].tobytes() for k in range(4)):
            return False
    return True
