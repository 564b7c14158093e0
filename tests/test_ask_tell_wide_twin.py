"""The CPU twin of the ask/tell L-BFGS kernel above n = 256 (tests/ask_tell_wide/atw_twin.hpp), without a GPU.

1. Fed the oracle's functors in the strided order of the kernel's threads (atw_lib.evaluate: oracle_lib.evaluate does not
   know that order, see there), the twin stepper equals
   oracle.minimize_batch(reduction="strided", width=T) — the twin of the persistent wide kernel — bit for bit on x, f, g
   and every progress field: the phase machine cut at the evaluation IS Lbfgs::Minimize in that order.
2. The f / g rows of finished problems are never read: NaN and 1e300 written over them change nothing.
3. The twin's own loop (atw_drive, the oracle's functors in C++) gives the same results: the GPU tests use it.
4. The inputs of the GPU test's torch objective are cleared here: on them the twin, fed numpy's evaluation of the same
   function, ends every problem on the gradient test with max |x| <= 1e-8."""
import numpy as np
import pytest

import at_lib
import atw_lib
import oracle_lib


@pytest.mark.parametrize("stop_name", ["default", "parity"])
@pytest.mark.parametrize("objective,n,m,B", atw_lib.TWIN_CASES)
def test_stepper_equals_the_strided_oracle(objective, n, m, B, stop_name):
    stop = atw_lib.stops()[stop_name]
    params = at_lib.params_of(objective, n)
    x0 = at_lib.starts(objective, B, n, seed=500 + n)
    got = atw_lib.twin_minimize(objective, x0, m, stop, params=params)
    want = atw_lib.oracle_minimize(objective, x0, m, stop, params=params)
    at_lib.assert_same_results(got, want, "%s n=%d m=%d %s" % (objective, n, m, stop_name))
    assert got[4] >= int(want[3]["nfev"].max())
    driven = atw_lib.twin_minimize_driven(objective, x0, m, stop, params=params)
    at_lib.assert_same_results(driven, want, "driven")
    assert driven[4] == got[4]


@pytest.mark.parametrize("poison", [np.nan, 1e300])
def test_rows_of_finished_problems_are_never_read(poison):
    objective, n, m, B = atw_lib.TWIN_CASES[2]
    stop = atw_lib.stops()["parity"]
    params = at_lib.params_of(objective, n)
    x0 = at_lib.starts(objective, B, n, seed=500 + n)
    x0[::2] *= 1e-3   # (every other problem starts close: the batch finishes over several rounds)
    want = atw_lib.oracle_minimize(objective, x0, m, stop, params=params)
    assert len(set(want[3]["nfev"].tolist())) > 1, "the problems finish in the same round: nothing would be poisoned"
    got = atw_lib.twin_minimize(objective, x0, m, stop, params=params, poison_finished=poison)
    at_lib.assert_same_results(got, want, "poison %r" % poison)


def test_hostile_starts_equal_the_strided_oracle():
    """NaN / inf coordinates, the minimiser itself (the search refused at once: the no-evaluation phase), 1e200"""
    n, m = 400, 6
    stop = at_lib.base_stop(num_iterations=40)
    x0 = np.concatenate([oracle_lib.hostile_starts(n), np.ones((2, n)), at_lib.starts("rosenbrock", 2, n, seed=3)])
    got = atw_lib.twin_minimize_driven("rosenbrock", x0, m, stop)
    at_lib.assert_same_results(got, atw_lib.oracle_minimize("rosenbrock", x0, m, stop), "hostile", nan_equal=True)


@pytest.mark.parametrize("n", atw_lib.TORCH_DIMS)
def test_torch_case_inputs_reach_the_gradient_stop(n):
    a, x0 = atw_lib.torch_case(n)
    stop = atw_lib.torch_case_stop()
    t = atw_lib.Twin(x0, 10, stop)

    def fn(X):
        return (a * X * X).sum(axis=1) + atw_lib.TORCH_C, 2.0 * a * X

    at_lib.drive(t, fn)
    x, f, g, p = t.results()
    assert np.all(p["status"] == atw_lib.GRADIENT_STATUS), p["status"]
    # at the stop |2 a_j x_j| < 1e-8 max(1, max |x|) with a_j >= 0.5, so |x_j| < 1e-8
    assert float(np.abs(x).max()) <= 1e-8


@pytest.mark.parametrize("objective", ["rosenbrock", "diag_quadratic"])
def test_strided_evaluation_is_the_oracles(objective):
    """atw_lib.evaluate is the oracle's functor in the strided order.  Up to n = width a lane holds one term, the strided
    order is the butterfly order, and oracle_lib.evaluate gives the same bits.  Above it: the f and g that
    oracle.minimize_batch(reduction="strided") returns with its final x (one iteration under a gradient test that fires at
    once) are this evaluation of that x."""
    n = 256
    x = at_lib.starts(objective, 3, n, seed=9)
    params = at_lib.params_of(objective, n)
    f, g = atw_lib.evaluate(objective, x, params=params, width=256)
    for b in range(3):
        fo, go = oracle_lib.evaluate(objective, x[b], params=params, reduction="butterfly", width=256)
        assert at_lib.same_bits(f[b], fo).all() and at_lib.same_bits(g[b], go).all()
    n = 700
    x = at_lib.starts(objective, 3, n, seed=10)
    params = at_lib.params_of(objective, n)
    f, g = atw_lib.evaluate(objective, x, params=params)
    stop = oracle_lib.make_stop(gradient_norm=1e300, gradient_norm_relative=0, past=0, x_delta=0.0, f_delta=0.0)
    xo, fo, go, po = atw_lib.oracle_minimize(objective, x, 4, stop, params=params)
    assert np.all(po["num_iterations"] == 1) and np.all(po["nfev"] >= 2)
    f1, g1 = atw_lib.evaluate(objective, xo, params=params)
    assert at_lib.same_bits(f1, fo).all() and at_lib.same_bits(g1, go).all()
