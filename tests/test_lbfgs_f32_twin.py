"""CPU tests of the native fp32 L-BFGS path's twin (tests/lbfgs_f32/f32_twin.hpp): in reference order it is the
reference's Lbfgs<F, m, MoreThuente> on float functors bit for bit — on the recorded file always, on a fresh draw where
the reference tree exists; it meets the reference's own end-to-end criterion; the gap between its two summation orders
is measured; its sanitizer build runs clean."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import l32_cases as Cs
import l32_lib as L


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    if not os.path.exists(L.TWIN_LIB):
        ge.build()


def twin_record(case):
    x, f, g, prog = L.twin_solve(case["objective"], case["m"], case["x0"], case["params"], case["stop"], order=L.REF_ORDER)
    _, _, _, _, rows, xs = L.twin_trajectory(case["objective"], case["m"], case["x0"][0], case["params"], case["stop"],
                                             order=L.REF_ORDER)
    return Cs.record_of(case, x, f, g, prog, rows, xs)


def check_overflow(got, want):
    """the overflowing start ends in NaNs whose bits belong to the processor: status, counts and NaN-ness"""
    for fld in ("status", "num_iterations", "nfev"):
        assert np.array_equal(got["progress"][fld], want["progress"][fld]), fld
    for fld in ("x_delta", "f_delta", "gradient_norm"):
        a, b = got["progress"][fld], want["progress"][fld]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), fld
    assert np.array_equal(np.isnan(got["f"]), np.isnan(want["f"]))
    assert np.array_equal(got["iterations0"], want["iterations0"])


def compare(cases, reference_of):
    wrong = []
    for case in cases:
        got, want = twin_record(case), reference_of(case)
        if case["name"].startswith("overflow"):
            check_overflow(got, want)
            continue
        want = {k: v for k, v in want.items()}
        got["progress"] = got["progress"].copy()
        got["progress"]["sum_k"] = want["progress"]["sum_k"]   # (not observable from outside the reference's step)
        bad = Cs.same_record(case, got, want)
        if bad:
            wrong.append((case["name"], bad))
    assert not wrong, "%d cases differ from the reference, first: %s" % (len(wrong), wrong[:5])


def test_twin_in_reference_order_is_the_recorded_reference():
    """x, f, g, every progress field, nfev and every per-iteration row and iterate of start 0, bit for bit."""
    cases = Cs.all_cases()
    recorded = Cs.load_recorded(cases)
    assert len(cases) == 2 * len(Cs.DIMS) * len(Cs.HISTORIES) * len(Cs.STOPS) + 2
    compare(cases, lambda c: recorded[c["name"]])


@pytest.mark.skipif(not os.path.isdir(L.REFERENCE), reason="needs the reference tree")
def test_twin_in_reference_order_is_the_reference_on_a_fresh_draw():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_f32", os.path.join(L.HERE, "golden", "make_golden_f32.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    seed = int.from_bytes(os.urandom(4), "little")
    print("fresh draw: seed", seed)
    with tempfile.TemporaryDirectory() as tmp:
        ref = L.reference_solver(L.build_reference(tmp))
        compare(Cs.all_cases(seed), lambda c: gen.reference_record(ref, c))


def test_reference_end_to_end_criterion():
    """EXPECT_NEAR(0, f, 1e-4) of the reference's verify.cc from (15, 8) and (-1, 2) on 2-D Rosenbrock, both orders."""
    for order in (L.REF_ORDER, L.DEVICE_ORDER):
        _, f, _, prog = L.twin_solve(L.ROSENBROCK, 10, Cs.VERIFY_STARTS, order=order)
        print("order", order, "f", f, "iterations", prog["num_iterations"], "status", prog["status"])
        assert np.all(np.abs(f) < Cs.VERIFY_BOUND)


def test_gap_between_the_two_orders():
    """A measurement between the twin's two policies (printed; l32_cases.ORDER_GAP_X / ORDER_GAP_F record it, and the
    recorded figures may not be smaller than what this draw gives: GPU test 5 is held to twice them)."""
    gap_x = gap_f = 0.0
    for case in Cs.all_cases():
        if not Cs.compared_as_numbers(case):
            continue
        a = L.twin_solve(case["objective"], case["m"], case["x0"], case["params"], case["stop"], order=L.REF_ORDER)
        b = L.twin_solve(case["objective"], case["m"], case["x0"], case["params"], case["stop"], order=L.DEVICE_ORDER)
        gap_x = max(gap_x, float(np.abs(a[0].astype(np.float64) - b[0]).max()))
        gap_f = max(gap_f, float(np.abs(a[1].astype(np.float64) - b[1]).max()))
    print("max |dx|_inf = %.7e, max |df| = %.7e" % (gap_x, gap_f))
    assert gap_x <= Cs.ORDER_GAP_X and gap_f <= Cs.ORDER_GAP_F
    assert gap_x >= 0.99 * Cs.ORDER_GAP_X and gap_f >= 0.99 * Cs.ORDER_GAP_F, "the recorded gap is stale"


def test_sanitize_target_runs_clean():
    out = subprocess.run(["make", "-s", "-C", L.L32_DIR, "sanitize"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert out.stdout.count("status") == 6
