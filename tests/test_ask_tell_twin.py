"""The CPU twin of the ask/tell L-BFGS stepper (tests/ask_tell/at_twin.hpp) against the oracle's Lbfgs::Minimize.

Fed the oracle's own evaluation as the callback, problem by problem, the stepper must return oracle_lib.minimize_batch
bit for bit — x, f, g and every progress field, nfev included — in the sequential order (the order pinned to the
reference's headers: the resumable search IS the reference's algorithm) and in the butterfly order at the widths of the
device mappings (the order tests/test_gpu_ask_tell.py holds the device to).  The last tests clear the inputs of that
module's torch-objective comparison: the gap between the twin's two orders stays inside the project's 1e-6 envelope."""
import numpy as np
import pytest

import at_lib
import oracle_lib

ORDERS = (("sequential", at_lib.SEQUENTIAL), ("butterfly", at_lib.BUTTERFLY))


def check(objective, x0, m, stop, widths=None, poison_finished=None):
    n = x0.shape[1]
    params = at_lib.params_of(objective, n)
    for reduction, order in ORDERS:
        for width in (widths or (at_lib.padded_width(n),)) if order == at_lib.BUTTERFLY else (at_lib.padded_width(n),):   # (unused by the sequential order)
            want = oracle_lib.minimize_batch(objective, x0, m=m, stop=stop, params=params, reduction=reduction, width=width)
            got = at_lib.twin_minimize(objective, x0, m, stop, params=params, order=order, width=width,
                                       poison_finished=poison_finished)
            at_lib.assert_same_results(got, want, "%s n=%d m=%d %s width=%d" % (objective, n, m, reduction, width))
            # one evaluation per round and problem at most: rounds bound nfev from above
            assert got[4] >= int(want[3]["nfev"].max())


@pytest.mark.parametrize("n", at_lib.DIMS)
@pytest.mark.parametrize("objective", ["rosenbrock", "diag_quadratic"])
def test_stepper_equals_minimize(objective, n):
    for m in at_lib.HISTORIES:
        check(objective, at_lib.starts(objective, 6, n, seed=100 * n + m), m, at_lib.base_stop())


@pytest.mark.parametrize("n,widths", [(13, (16, 32, 64, 128, 256)), (130, (256,))])
def test_stepper_at_every_device_width(n, widths):
    check("rosenbrock", at_lib.starts("rosenbrock", 4, n, seed=7), 6, at_lib.base_stop(), widths=widths)


@pytest.mark.parametrize("name", sorted(at_lib.stop_records()))
def test_stopping_records(name):
    stop = at_lib.stop_records()[name]
    for objective, n, m in (("rosenbrock", 13, 6), ("diag_quadratic", 33, 3)):
        check(objective, at_lib.starts(objective, 8, n, seed=31), m, stop)


def test_stopping_records_cover_the_plateau_ring_and_the_iteration_limit():
    records = at_lib.stop_records()
    assert any(s.past > 0 for s in records.values())
    x0 = at_lib.starts("rosenbrock", 8, 13, seed=31)
    got = at_lib.twin_minimize("rosenbrock", x0, 6, records["everything_off_but_limit"])
    assert np.all(got[3]["status"] == 1) and np.all(got[3]["num_iterations"] == 31)
    got = at_lib.twin_minimize("rosenbrock", x0, 6, records["past8"])
    assert np.any(got[3]["status"] == 3)


@pytest.mark.parametrize("n", [5, 13, 65])
@pytest.mark.parametrize("objective", ["rosenbrock", "diag_quadratic"])
def test_hostile_starts(objective, n):
    """NaN / inf coordinates and overflowing magnitudes: the non-finite bail-out and the refused-search path"""
    check(objective, oracle_lib.hostile_starts(n), 6, at_lib.base_stop(num_iterations=40))


def test_refused_search_path_is_reached():
    """a start at the minimiser: g = 0, the fallback direction has g.g = 0 >= 0 and the search is refused at once"""
    x0 = np.ones((2, 8))
    got = at_lib.twin_minimize("rosenbrock", x0, 6, at_lib.base_stop())
    want = oracle_lib.minimize_batch("rosenbrock", x0, m=6, stop=at_lib.base_stop())
    at_lib.assert_same_results(got, want)
    assert np.all(got[3]["nfev"] == 1) and np.all(got[3]["num_iterations"] == 1) and got[4] == 2


@pytest.mark.parametrize("poison", [float("nan"), 1e300])
def test_rows_of_finished_problems_are_never_read(poison):
    x0 = at_lib.starts("rosenbrock", 16, 13, seed=5)
    x0[3] = 1.0   # finishes in the second round
    check("rosenbrock", x0, 6, at_lib.base_stop(), poison_finished=poison)


@pytest.mark.parametrize("objective,n,m", at_lib.TORCH_CASES)
def test_cross_order_gap_of_the_gpu_inputs(objective, n, m):
    """The inputs of the GPU module's torch-objective comparison: the twin's two orders are within the project's stated
    envelope (README "Parity") of each other, and their statuses agree on all but 2 % of the batch."""
    x0 = at_lib.torch_case_inputs(objective, n)
    params = at_lib.params_of(objective, n)
    stop = at_lib.torch_case_stop()
    seq = oracle_lib.minimize_batch(objective, x0, m=m, stop=stop, params=params, reduction="sequential")
    but = oracle_lib.minimize_batch(objective, x0, m=m, stop=stop, params=params, reduction="butterfly",
                                    width=at_lib.padded_width(n))
    # (the stepper in either order equals these bit for bit: checked on a slice, the whole batch above would be slow)
    for order, want in ((at_lib.SEQUENTIAL, seq), (at_lib.BUTTERFLY, but)):
        got = at_lib.twin_minimize(objective, x0[:4], m, stop, params=params, order=order,
                                   width=at_lib.padded_width(n))
        at_lib.assert_same_results(got, tuple(a[:4] for a in want), "slice")
    dx = float(np.max(np.abs(seq[0] - but[0])))
    df = float(np.max(np.abs(seq[1] - but[1])))
    disagree = int(np.count_nonzero(seq[3]["status"] != but[3]["status"]))
    print("cross-order gap %s n=%d m=%d: max|dx| %.3g max|df| %.3g, statuses that differ %d of %d"
          % (objective, n, m, dx, df, disagree, len(x0)))
    assert dx <= at_lib.CONTRACT and df <= at_lib.CONTRACT
    assert disagree <= at_lib.MAX_STATUS_DISAGREEMENT * len(x0)
