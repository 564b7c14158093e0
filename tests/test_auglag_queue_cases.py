"""The inputs of tests/test_gpu_auglag_queue.py, checked on the CPU oracle: the conditions that make the capped device
runs mean something are properties of the batches (tests/alq_cases.py) and of what the oracle computes on them, so they
are cleared here without a GPU; the device test asserts them again from the same oracle call.

  * every batch holds at least four problems per resident problem slot under its largest cap, is no multiple of the
    segments of a wavefront, has its penalties spread over three decades or more and its degenerate rows each followed
    by an ordinary one;
  * the convergent batches end with status 6 on every row, after numbers of outer iterations that differ by 8 or more;
  * the lock-step batches have survivors past outer iteration 8 (the chain-of-four launches) and, at n = 7, past 32
    (the second half-ring of counters is zeroed);
  * the hand-over batch: more than 256 survivors after outer iteration 4, the first read-back with 1..256 survivors is
    one of 8, 12, 16, ..., it hands at least three rows per problem slot of a workgroup to the fused kernel, and no row
    ends on the iteration limit.  The schedule is printed."""
import numpy as np
import pytest

import alq_cases as A


def _all_cases():
    cases = [A.fused_mixed(n) for n in A.FUSED_N] + [A.fused_convergent(n) for n in (7, 40)]
    cases += [A.fused_box(n, b) for n in A.BOX_N for b in ("set", "never_set")]
    cases += [A.fused_hager_zhang(12), A.fused_hager_zhang(40), A.fused_box(12, "set", "hager_zhang", caps=(1, 3))]
    cases += [A.fused_family()] + [A.lockstep(i, n) for i, n in A.LOCKSTEP] + [A.handover(), A.device_entry()]
    cases += [A.user_terms("fused"), A.user_terms("lockstep")]
    return cases


def test_batches_refetch_under_their_caps_and_are_mixed():
    names = set()
    for case in _all_cases():
        A.check_batch(case)
        assert case.name not in names
        names.add(case.name)
        assert case.oracle_rows.size >= 16 and (case.n > 64 or case.oracle_rows.size == case.B)
        assert case.B == A.smallest_batch(case.launch, max(case.caps)) or case.name == "handover_7"
    # starts on a bound, and a corner, where the bounds are set
    for case in [A.fused_box(n, "set") for n in A.BOX_N] + [A.lockstep("lbfgsb", 12)]:
        on = (case.x0 == case.lower) | (case.x0 == case.upper)
        assert on.any(axis=1).sum() >= 4 and on.all(axis=1).any(), case.name


def test_degenerate_rows_and_limits_in_the_mixed_batch():
    """The smallest mixed batch on the oracle: the rows of NaN, with a +inf and with a -inf coordinate stop in their first
    outer iteration (the row of NaN as "finished": a NaN never wins the comparisons of the violation and KKT norms), the
    others run into the outer iteration limit after inner solves of very different lengths; a row that stops at once is
    followed by one that runs to the limit and the other way round."""
    case = A.fused_mixed(7)
    pr = A.oracle(case)["progress"]
    limit = case.cfg_kw["outer_num_iterations"]
    at_once = case.spliced[[0, 2, 3]]
    assert (pr["num_iterations"][at_once] == 1).all() and pr["status"][at_once].tolist() == [6, 1, 1]
    rest = np.delete(np.arange(case.B), at_once)
    assert (pr["num_iterations"][rest] == limit + 1).all() and (pr["status"][rest] == 1).all()
    inner = pr["inner_iterations"][rest]
    print("%s: inner iterations of the rows that run to the limit %d .. %d" % (case.name, inner.min(), inner.max()))
    assert inner.max() >= 4 * inner.min()
    assert 0 < at_once[1] < case.B - 1            # ... with rows that run to the limit on both sides


@pytest.mark.parametrize("n", [7, 40])
def test_convergent_batches_converge_after_very_different_numbers_of_iterations(n):
    case = A.fused_convergent(n)
    pr = A.oracle(case)["progress"]
    its = pr["num_iterations"]
    print("%s: B = %d, outer iterations %d .. %d" % (case.name, case.B, its.min(), its.max()))
    assert (pr["status"] == 6).all()
    assert its.min() >= 2 and its.max() >= its.min() + 8 and its.max() <= case.cfg_kw["outer_num_iterations"]


@pytest.mark.parametrize("inner,n", sorted(A.LOCKSTEP))
def test_lockstep_batches_have_survivors_in_the_chain_of_four_regime(inner, n):
    case = A.lockstep(inner, n)
    its = A.oracle(case)["progress"]["num_iterations"]
    print("%s: B = %d, survivors after 4, 8, 32: %d, %d, %d" % (case.name, case.B, A.survivors(its, 4),
                                                               A.survivors(its, 8), A.survivors(its, 32)))
    assert A.survivors(its, 8) > 0
    if case.cfg_kw["outer_num_iterations"] > 32:
        assert A.survivors(its, 32) > 0


def test_handover_schedule():
    case = A.handover()
    A.check_batch(case)
    o = A.oracle(case)
    schedule, r = A.check_handover_conditions(case, o)
    its = o["progress"]["num_iterations"]
    print("%s: B = %d, outer iterations %d .. %d; survivors at the read-backs: %s; hand-over after iteration %d with %d "
          "rows on %d slots per workgroup" % (case.name, case.B, its.min(), its.max(),
                                              ", ".join("rem(%d) = %d" % s for s in schedule), r, schedule[-1][1],
                                              case.slots))


def _result(x, lam):
    B = x.shape[0]
    pr = np.zeros(B, dtype=A.al.PROGRESS_DTYPE)
    pr["f_delta"] = np.nan
    return {"x": x, "lambda": lam, "mu": np.zeros((B, 0)), "penalty": np.ones(B), "max_violation": np.zeros(B),
            "max_lagrangian_gradient": np.zeros(B), "progress": pr}


def test_the_comparison_is_bit_for_bit():
    """first_difference: a zero of the other sign, a last-bit change and a NaN against a number are differences; a NaN of
    the other sign is one between two device runs and none against the oracle; a field without columns compares equal."""
    x = np.array([[0.0, 1.0], [np.nan, 2.0], [3.0, 4.0]])
    lam = np.array([[0.5], [0.25], [0.125]])
    a = _result(x, lam)
    assert A.first_difference(a, _result(x.copy(), lam.copy())) is None
    for row, col, value in ((0, 0, -0.0), (2, 1, np.nextafter(4.0, 5.0)), (1, 0, 7.0), (2, 0, np.nan)):
        y = x.copy()
        y[row, col] = value
        for any_nan in (False, True):
            diff = A.first_difference(a, _result(y, lam), slots=2, any_nan=any_nan)
            assert diff is not None and diff.startswith("x differs in 1 of 3 rows, first rows [%d]" % row), diff
    y = x.copy()
    y[1, 0] = -np.nan
    assert np.signbit(y[1, 0]) != np.signbit(x[1, 0])
    assert A.first_difference(a, _result(y, lam), any_nan=True) is None
    assert A.first_difference(a, _result(y, lam)).startswith("x differs in 1 of 3 rows, first rows [1]")
    b = _result(x, lam)
    b["progress"]["nfev"][2] = 1
    assert A.first_difference(a, b, any_nan=True).startswith("progress.nfev differs in 1 of 3 rows, first rows [2]")
