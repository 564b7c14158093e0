"""The condition-number brackets on the CPU (tests/cond_cases.py): what tests/test_gpu_condition_value.py relies on.

  * cond_cases.condition is the twins' `condition` bit for bit (nd_twin.hpp and tr_twin.hpp), so its mutants are mutants
    of the twin.
  * Every planted bug lies OUTSIDE the bracket [c (1 - delta), c (1 + delta)] wherever it changes the computed real
    number — and where a bug does not change that number the file says so and asserts that instead (MUTANTS below): two
    of the five are other orders of computing the same number, which no threshold on the value can see.
  * The generator conditions: after the first iterate the twin of every case is in status CONTINUE with a finite x1; every
    bracketed condition number is finite and below 1e15; where the Hessian differs from problem to problem no two of a
    batch lie within 4 delta of each other.
  * The host Hessians are the 200-bit Hessians of tests/hp_lib.py within that file's bound, and the twins' condition
    number of them is the 200-bit ||H||_F ||H^-1||_F within the bound of tests/test_dense_lu_mpmath.py (n <= 17)."""
import math

import mpmath
import numpy as np
import pytest

import cond_cases as K
import hp_lib as HP
import nd_lib as T
import test_dense_lu_mpmath as L
import tr_lib

SOLVERS = ("newton_descent", "trust_region")


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _finite(c):
    return math.isfinite(c)


# ---- the numpy copy is the twin ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", K.ALL_DENSE_DIMS)
def test_numpy_condition_is_both_twins_bit_for_bit(n):
    for name, S in K.dense_matrices(n):
        c = K.condition(S)
        assert _same(c, T.twin_condition(S)), name
        assert _same(c, L.tr_twin_condition(S)), name
        assert K.Factorisation(S).piv == T.twin_lu(S)[1].tolist(), name
    for x in K.rosenbrock_starts(n):
        H = K.rosenbrock_hessian(x)
        assert _same(K.condition(H), T.twin_condition(H))


def test_dense_matrices_hold_what_the_lu_must_meet():
    """pivots 8 and 32 rows away, exact first-column ties, interchanges with fill-in behind them, H != H^T, indefinite
    matrices, condition numbers from 1e1 to 1e12 — and the singular one is singular in the first column"""
    far8 = far32 = ties = asymmetric = 0
    for n in K.ALL_DENSE_DIMS:
        conds = []
        for name, S in K.dense_matrices(n):
            F = K.Factorisation(S)
            if name == K.SINGULAR:
                assert not S[:, 0].any() and not S[0, :].any() and not _finite(K.condition(S))
                continue
            far8 += F.max_pivot_distance >= 8
            far32 += F.max_pivot_distance >= 32
            ties += F.first_column_ties
            asymmetric += name.startswith("asymmetric") and S.tobytes() != np.ascontiguousarray(S.T).tobytes()
            if name.startswith("indefinite"):
                assert np.linalg.eigvalsh(S).min() < 0 < np.linalg.eigvalsh(S).max(), (n, name)
            if name.startswith("random, "):
                conds.append(K.condition(S))
            if n >= 7:
                assert np.count_nonzero(np.triu(F.lu, 1)) >= 0.9 * n * (n - 1) / 2, (n, name, "U is not dense")
        assert min(conds) < 2e2 and max(conds) > 1e11, (n, conds)
    assert far8 >= 10 and far32 >= 4 and ties >= 10 and asymmetric >= 5, (far8, far32, ties, asymmetric)


# ---- the brackets see a wrong kernel -----------------------------------------------------------------------------------


# The pivot mutant shows where the condition number is at least this (see MUTANTS): the planted-tie random matrices of
# condition 1e8 and 1e12 at n >= 7 are above it (1e7 and more), every recorded tie matrix is below (2.5e5 at most), and so
# are the two n = 2 ones, where planting the tie replaced the small singular value (6.5 and 21)
PIVOT_MUTANT_SHOWS_FROM = 1e6


# mutation -> (changes(n, W, name, S, F): whether the bug changes the real number computed on this matrix, reason for
# the matrices where it does not)
MUTANTS = {
    K.LAST_INVERSE_COLUMN_DROPPED: (
        lambda n, W, name, S, F: True,
        "no matrix: a column of an inverse is never zero"),
    K.SECOND_ROW_NOT_UPDATED: (
        lambda n, W, name, S, F: n >= W + 2,
        "n <= W + 1: the trailing block of step 0 has n - 1 <= W rows, one per lane; no lane ever owns a second"),
    K.BUTTERFLY_LEVEL_DROPPED: (
        lambda n, W, name, S, F: True,
        "no matrix: the odd lanes hold t = 1, 3, ...: H(1, 0) among them, which is non-zero on every matrix here"),
    # A tie broken the other way is another exact factorisation P' A = L' U' of the same matrix: the real number is the
    # same and only its rounding moves, by something of the order n u cond of the value (test_dense_lu_mpmath.py).  The
    # bracket is (2 n^2 + 8) u wide, so it can see the bug only where the condition number is large against n: asserted
    # from PIVOT_MUTANT_SHOWS_FROM on (measured there: 5e5 u and more).  Below it the recorded tie matrices (small
    # integers times powers of two) move by 2 .. 60 u: inside.  The device's tie-break at those sizes is pinned
    # elsewhere: tests/test_gpu_condition_value.py runs the planted-tie matrices on all three
    # kernels, and the solve LU's pivot order on the recorded ties is held by the Newton-descent goldens.
    K.PIVOT_LAST_MAXIMUM: (
        lambda n, W, name, S, F: F.ties > 0 and K.condition(S) >= PIVOT_MUTANT_SHOWS_FROM,
        "tie-free matrices: first and last maximum coincide; tie matrices of condition below 1e6: another factorisation "
        "of the same matrix whose rounding differs by less than the bracket"),
    # The interchanges applied in order send e_c to e_sigma(c), sigma a permutation: without them the W-at-a-time loop
    # solves for the same n unit vectors in another order, and the sum of squares of the same n^2 numbers is the same up
    # to the order of summation — which is what delta allows.  No matrix can show it: ||A^-1 P||_F = ||A^-1||_F.
    K.INTERCHANGES_SKIPPED: (
        lambda n, W, name, S, F: False,
        "every matrix: the columns of the inverse come out permuted, their Frobenius norm is the same number"),
}


@pytest.mark.parametrize("mutation", K.MUTATIONS)
def test_mutant_lies_outside_the_bracket_wherever_it_changes_the_number(mutation):
    changes, reason = MUTANTS[mutation]
    seen = hidden = 0
    for n in K.ALL_DENSE_DIMS:
        W = K.two_row_width(n)
        for name, S in K.dense_matrices(n):
            if name == K.SINGULAR:
                continue
            c = K.condition(S)
            assert _finite(c) and c < K.MAX_CONDITION, (n, name)
            assert K.inside(c, c, n)
            v = K.condition(S, mutation, W)
            F = K.Factorisation(S)
            if changes(n, W, name, S, F):
                seen += 1
                assert not K.inside(v, c, n), "%s: n = %d, %s: %r inside the bracket of %r" % (mutation, n, name, v, c)
            else:
                hidden += 1
                # not a gap left open silently: on these matrices the mutant computes the same real number (`reason`),
                # and its value must then be inside — otherwise the reason is wrong
                assert K.inside(v, c, n), "%s: n = %d, %s: outside although %s" % (mutation, n, name, reason)
    print("%s: outside its bracket on %d matrices, the same number on %d (%s)" % (mutation, seen, hidden, reason))
    if mutation != K.INTERCHANGES_SKIPPED:
        assert seen >= 10, (mutation, seen)
    if mutation in (K.LAST_INVERSE_COLUMN_DROPPED, K.BUTTERFLY_LEVEL_DROPPED):
        assert hidden == 0


def test_pivot_mutant_changes_the_pivots_on_every_tie_matrix():
    """... so where it stays inside the bracket it is not for lack of a tie"""
    ties = 0
    for n in K.ALL_DENSE_DIMS:
        for name, S in K.dense_matrices(n):
            F = K.Factorisation(S)
            if name != K.SINGULAR and F.ties:
                ties += 1
                assert K.Factorisation(S, K.PIVOT_LAST_MAXIMUM).piv != F.piv, (n, name)
            elif name != K.SINGULAR:
                assert _same(K.condition(S, K.PIVOT_LAST_MAXIMUM), K.condition(S)), (n, name)
    assert ties >= 20


# ---- generator conditions ----------------------------------------------------------------------------------------------


def _only_the_limit(lib, limit):
    return lib.make_stop(num_iterations=limit, x_delta_violations=1, f_delta_violations=1)


def _twin(solver, objective, x0, params, limit, condition_stop, W):
    if solver == "newton_descent":
        return T.twin_solve(objective, x0, params, _only_the_limit(T, limit), None, condition_stop, order=T.DEVICE_ORDER,
                            W=W)
    return tr_lib.twin_solve(objective, x0, params, _only_the_limit(tr_lib, limit), None, condition_stop,
                             order=tr_lib.DEVICE_ORDER, W=W)


def twin_first_iterate(solver, objective, x0, params, W, must_stop=True):
    """x1 of the twin, with the generator conditions on the solve: under a stop record in which only the iteration limit
    is active the solve runs past iterate 1 (limit 1: it ends on the limit with num_iterations == 2 — no other stop test,
    no bail-out, no rejected step ended it), and x1 is finite.  x1 itself is what the twin returns when a threshold
    below every condition number stops it at its first test."""
    _, _, _, p = _twin(solver, objective, x0, params, 1, 0.0, W)
    assert (p["status"] == K.ITERATION_LIMIT).all() and (p["num_iterations"] == 2).all(), (solver, p["status"])
    x1, _, _, p1 = _twin(solver, objective, x0, params, 5, 1e-300, W)
    if must_stop:
        assert (p1["status"] == K.CONDITION).all() and (p1["num_iterations"] == 1).all(), (solver, p1["status"])
        assert np.isfinite(x1).all()
    return x1, p1


def _check_values(cs, n, per_problem, what):
    assert all(_finite(c) and c < K.MAX_CONDITION for c in cs), (what, cs)
    if per_problem:
        assert K.separated(cs, n), (what, cs)
    for c in cs:
        lo, hi = K.thresholds(c, n)
        assert lo < c * (1 - K.delta(n) / 2) and hi > c * (1 + K.delta(n) / 2) and lo > 0


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("n,W", K.NEWTON_PAIRS)
def test_generator_conditions_rosenbrock_and_diag_quadratic(solver, n, W):
    x0 = K.rosenbrock_starts(n)
    if n == 1:
        # H = (0): the twin's value is NaN, the test can never fire, and x1 is whatever the limit returns
        twin_first_iterate(solver, T.ROSENBROCK, x0, None, W, must_stop=False)
        assert math.isnan(T.twin_condition(K.rosenbrock_hessian(x0[0])))
    else:
        x1, _ = twin_first_iterate(solver, T.ROSENBROCK, x0, None, W)
        _check_values([T.twin_condition(K.rosenbrock_hessian(x)) for x in x1], n, True, (solver, "rosenbrock", n))
    for indefinite in (False, True):
        a, c, q0 = K.diag_quadratic_inputs(n, indefinite)
        twin_first_iterate(solver, T.DIAG_QUADRATIC, q0, np.concatenate([a, [c]]), W)
        _check_values([T.twin_condition(K.diag_quadratic_hessian(a))], n, False, (solver, "diag", n, indefinite))
    if n == 1:
        a, _, _ = K.diag_quadratic_inputs(1, False)
        assert T.twin_condition(K.diag_quadratic_hessian(a)) == 1.0 == L.tr_twin_condition(K.diag_quadratic_hessian(a))


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("n", K.DENSE_DIMS)
def test_generator_conditions_dense(solver, n):
    x0, b = K.dense_starts(n), K.dense_rhs(n)
    for name, S in K.dense_matrices(n):
        p = K.dense_params(S, b, 0.0)
        if name == K.SINGULAR:
            c = T.twin_condition(S)
            assert not _finite(c) and _same(c, L.tr_twin_condition(S))
            continue
        twin_first_iterate(solver, T.DENSE, x0, p, None)
        _check_values([T.twin_condition(S)], n, False, (solver, n, name))
    p, x0 = K.kappa_batch(n)
    x1, _ = twin_first_iterate(solver, T.DENSE, x0, p, None)
    _check_values([T.twin_condition(K.dense_hessian(p, x)) for x in x1], n, True, (solver, n, "kappa"))


@pytest.mark.parametrize("n", K.ROSENBROCK_DIMS)
def test_generator_conditions_lbfgs_rosenbrock(n):
    """The Lbfgs twin (the oracle in butterfly order at the padded width; the device test repeats the conditions on the
    device's own x1, whose last bits depend on the mapping)."""
    import oracle_lib
    W = T.padded_width(n)
    x0 = K.rosenbrock_starts(n)
    for ls in ("more_thuente", "hager_zhang"):
        stop = oracle_lib.make_stop(num_iterations=1, x_delta=0.0, f_delta=0.0, gradient_norm=0.0, past=0)
        _, _, _, p = oracle_lib.minimize_batch("rosenbrock", x0, stop=stop, second_mode="functor", linesearch=ls,
                                               reduction="butterfly", width=W)
        assert (p["status"] == K.ITERATION_LIMIT).all() and (p["num_iterations"] == 2).all(), (ls, p["status"])
        stop.num_iterations = 5
        oracle_lib.lib().oracle_set_condition_hessian_stop(1e-300)
        try:
            x1, _, _, p1 = oracle_lib.minimize_batch("rosenbrock", x0, stop=stop, second_mode="functor", linesearch=ls,
                                                     reduction="butterfly", width=W)
            co = oracle_lib.hessian_conditions(K.B)
        finally:
            oracle_lib.lib().oracle_set_condition_hessian_stop(0.0)
        assert (p1["status"] == K.CONDITION).all() and (p1["num_iterations"] == 1).all() and np.isfinite(x1).all()
        cs = [T.twin_condition(K.rosenbrock_hessian(x)) for x in x1]
        _check_values(cs, n, True, ("lbfgs", ls, n))
        # the Lbfgs twin's own condition numbers (the reference binary's bit for bit, tests/test_oracle.py) are these
        assert all(_same(a, b) for a, b in zip(co, cs)), (ls, n)


def _lbfgs_twin(x0, limit, condition_stop, n):
    import oracle_lib
    stop = oracle_lib.make_stop(num_iterations=limit, x_delta=0.0, f_delta=0.0, gradient_norm=0.0, past=0)
    oracle_lib.lib().oracle_set_condition_hessian_stop(condition_stop)
    try:
        return oracle_lib.minimize_batch("rosenbrock", x0, m=5, stop=stop, second_mode="functor", reduction="butterfly",
                                         width=T.padded_width(n))
    finally:
        oracle_lib.lib().oracle_set_condition_hessian_stop(0.0)


@pytest.mark.parametrize("solver", SOLVERS + ("lbfgs",))
def test_later_iterate_rows_are_the_ones_whose_condition_number_peaks_at_iterate_3(solver):
    """cond_cases.LATER_ITERATE_ROWS, on the twins: x1 from a threshold below every value, x2 and x3 from limits 1 and 2"""
    n, x0 = K.LATER_ITERATE_N, K.later_iterate_starts()
    if solver == "lbfgs":
        xs = [_lbfgs_twin(x0, 5, 1e-300, n)[0]] + [_lbfgs_twin(x0, limit, 0.0, n)[0] for limit in (1, 2)]
        assert (_lbfgs_twin(x0, 3, 0.0, n)[3]["num_iterations"] == 4).all()
    else:
        xs = [twin_first_iterate(solver, T.ROSENBROCK, x0, None, None)[0]] + \
             [_twin(solver, T.ROSENBROCK, x0, None, limit, 0.0, None)[0] for limit in (1, 2)]
        assert (_twin(solver, T.ROSENBROCK, x0, None, 3, 0.0, None)[3]["num_iterations"] == 4).all()
    c = np.array([[T.twin_condition(K.rosenbrock_hessian(x[b])) for x in xs] for b in range(len(x0))])
    rows = tuple(b for b in range(len(x0)) if K.thresholds(c[b, 2], n)[0] > max(c[b, :2]) * (1 + K.delta(n)))
    assert rows == K.LATER_ITERATE_ROWS[solver], (solver, rows, c)


# ---- the host Hessians and the twins' value against 200 bits -----------------------------------------------------------


def _assert_hessian(H, definition, magnitude, k, what):
    n = H.shape[0]
    for i in range(n):
        for j in range(n):
            ok, ratio = HP.within(H[i, j], definition[i][j], k, magnitude[i][j])
            assert ok, "%s: H(%d, %d) off by %s of its bound" % (what, i, j, mpmath.nstr(ratio, 5))


def _assert_condition(H, what):
    n = H.shape[0]
    ref = L.Elimination(H)
    with mpmath.workdps(50):
        cond = ref.condition()
        for fn in (T.twin_condition, L.tr_twin_condition):
            err = abs(mpmath.mpf(fn(H)) - cond) / cond
            assert err <= L.CONDITION_C[n] * n * L.U * cond, (what, float(err / (n * L.U * cond)), L.CONDITION_C[n])


@pytest.mark.parametrize("n", [m for m in K.ROSENBROCK_DIMS if m <= 17])
def test_rosenbrock_hessian_and_its_condition_against_200_bits(n):
    x1, _ = twin_first_iterate("newton_descent", T.ROSENBROCK, K.rosenbrock_starts(n), None, None)
    for b, x in enumerate(np.vstack([x1, K.rosenbrock_starts(n)])):
        H = K.rosenbrock_hessian(x)
        d = HP.rosenbrock(x, hessian=True)
        _assert_hessian(H, d.H, d.H_abs, HP.rosenbrock_k(n)[2], "rosenbrock n = %d row %d" % (n, b))
        assert HP.rosenbrock_k(n)[2] == 5
        _assert_condition(H, "rosenbrock n = %d row %d" % (n, b))


@pytest.mark.parametrize("n", [m for m in K.DENSE_DIMS if m <= 17])
def test_dense_and_diagonal_hessians_and_their_condition_against_200_bits(n):
    p, x0 = K.kappa_batch(n)
    x1, _ = twin_first_iterate("newton_descent", T.DENSE, x0, p, None)
    S, kappa = p[:n * n].reshape(n, n).T, HP.mpf(float(p[n * n + n]))
    for b, x in enumerate(x1):
        H = K.dense_hessian(p, x)
        # S(i, i) + (3 kappa)(x_i x_i): 3 kappa, x x, their product, the sum — a chain of 4 on the diagonal, 0 off it
        xs = HP.vec(x)
        d = [[HP.mpf(float(S[i, j])) + (3 * kappa * xs[i] * xs[i] if i == j else 0) for j in range(n)] for i in range(n)]
        m = [[abs(HP.mpf(float(S[i, j]))) + (3 * kappa * xs[i] * xs[i] if i == j else 0) for j in range(n)] for i in range(n)]
        _assert_hessian(H, d, m, 4, "dense n = %d row %d" % (n, b))
        _assert_condition(H, "dense n = %d row %d" % (n, b))
    for name, M in K.dense_matrices(n):
        if name != K.SINGULAR:
            assert K.dense_hessian(K.dense_params(M, K.dense_rhs(n), 0.0), x1[0]).tobytes() == M.tobytes(), name
            _assert_condition(M, "n = %d, %s" % (n, name))
    for indefinite in (False, True):
        a, c, q0 = K.diag_quadratic_inputs(n, indefinite)
        H = K.diag_quadratic_hessian(a)
        d = HP.diag_quadratic(q0[0], a, c, hessian=True)
        _assert_hessian(H, d.H, d.H_abs, HP.diag_quadratic_k(n)[2], "diag n = %d" % n)
        _assert_condition(H, "diag n = %d" % n)
