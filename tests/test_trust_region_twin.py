"""TrustRegionNewton on the CPU: the twin of the trust-region kernel in reference order (tests/trust_region/tr_twin.hpp)
against the reference's recorded solves, bit for bit, and — where the reference tree exists — against the reference
itself on a fresh draw compiled at test time; the C ABI's config defaults."""
import os
import re

import numpy as np
import pytest

import dense_cases as D
import tr_cases
import tr_lib as T

CASES = tr_cases.load_cases()
PROGRESS_FIELDS = ("status", "num_iterations", "nfev", "x_delta", "f_delta", "gradient_norm")


def assert_same(ref, twin, what):
    x, f, g, p = ref
    tx, tf, tg, tp = twin
    assert x.tobytes() == tx.tobytes(), what + ": x"
    assert f.tobytes() == tf.tobytes(), what + ": f"
    assert g.tobytes() == tg.tobytes(), what + ": g"
    for k in PROGRESS_FIELDS:
        assert p[k].tobytes() == tp[k].tobytes(), what + ": progress." + k


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_reference_order_matches_golden(case):
    twin = T.twin_solve(int(case["objective"]), case["x0"], case["params"], case["stop"], case["config"],
                        float(case["condition_stop"]), order=T.REF_ORDER)
    if "g" not in case:
        # a dense case: g* (and x* above n = 33) recorded as digests of the reference's bytes (dense_cases.py)
        assert D.same_as_recorded(case, "x", twin[0]), case["name"] + ": x"
        assert D.same_as_recorded(case, "g", twin[2]), case["name"] + ": g"
        case = {**case, "x": twin[0], "g": twin[2]}
    assert_same((case["x"], case["f"], case["g"], case["progress"]), twin, case["name"])


def test_golden_covers_the_quirks():
    by = {c["name"]: c for c in CASES}
    # a zero step gives rho = -inf: the radius shrinks from 1 to min_radius (20 trial points), then the stall
    assert (by["edge_at_minimiser"]["progress"]["nfev"] == 22).all()
    # an overflowing trial point (NaN rho) repeats the identical subproblem to the retry limit
    assert (by["edge_overflow_trial"]["progress"]["nfev"] == 52).all()
    # no retries: the step returns current, Progress sees x_delta = 0
    assert (by["edge_retry_limit_0"]["progress"]["x_delta"] == 0).all()
    # the indefinite quadratic is unbounded: iteration limit, finite values
    p = by["diag_quadratic_indefinite"]["progress"]
    assert (p["status"] == 1).all() and np.isfinite(by["diag_quadratic_indefinite"]["f"]).all()
    assert (by["edge_condition_hessian"]["progress"]["status"] == 5).any()


DENSE_CASES = [c for c in CASES if c["name"].startswith("dense_")]


def _twin_ex(case, order, **kw):
    return T.twin_solve_ex(int(case["objective"]), case["x0"], case["params"], case["stop"], case["config"],
                           float(case["condition_stop"]), order=order, **kw)


def test_dense_cases_reach_the_cg_and_the_condition_test():
    """What the generator asserted of the dense-Hessian cases, from the twin's counters today: CG runs of 3 iterations and
    more at n >= 33, negative-curvature exits and boundary hits on the indefinite family, at least 4 starts per case, and
    condition numbers away from the threshold, in both summation orders, with both decisions taken."""
    by = {c["name"]: c for c in DENSE_CASES}
    cnt = {nm: _twin_ex(c, T.REF_ORDER)[4] for nm, c in by.items()}
    for n in D.DIMS:
        for kind in ("dense_spd_n%02d_default", "dense_spd_n%02d_parity", "dense_asym_n%02d_default",
                     "dense_indefinite_n%02d_default"):
            assert 4 <= by[kind % n]["x0"].shape[0] <= 8 and by[kind % n]["x0"].shape[1] == n
    assert any(cnt["dense_spd_n%02d_default" % n]["max_cg_iterations"].max() >= 3 for n in D.DIMS if n >= 33)
    assert sum(int(v["negative_curvature_exits"].sum()) for k, v in cnt.items() if k.startswith("dense_indefinite_")) >= 1
    assert sum(int(v["boundary_hits"].sum()) for k, v in cnt.items() if k.startswith("dense_indefinite_")) >= 1
    for n in (9, 33, 64):
        name = "dense_condition_n%02d" % n
        status = by[name]["progress"]["status"]
        margin = min(cnt[name]["min_condition_margin"].min(),
                     _twin_ex(by[name], T.DEVICE_ORDER)[4]["min_condition_margin"].min())
        assert margin >= 1e-9, name
        assert (status == 5).any() and (status != 5).any(), (name, status)
        assert (by[name]["progress"]["num_iterations"][status == 5] >= 2).any(), name


@pytest.mark.parametrize("case", DENSE_CASES, ids=[c["name"] for c in DENSE_CASES])
def test_dense_device_order_within_the_contract(case):
    """This file marks no case: on every recorded dense row the twin's two summation orders end within 1e-6 in x* and f*
    with the same status, so the device can be held to the reference's record there."""
    import nd_cases
    assert not nd_cases.misses_contract(_twin_ex(case, T.REF_ORDER), _twin_ex(case, T.DEVICE_ORDER)).any()


ASYMMETRIC_CASES = [c for c in DENSE_CASES if c["name"].startswith("dense_asym_")]


@pytest.mark.parametrize("case", ASYMMETRIC_CASES, ids=[c["name"] for c in ASYMMETRIC_CASES])
def test_asymmetric_cases_notice_a_transposed_product(case):
    """H(i, j) != H(j, i) in the last bits: the twin with H d walking a column of H for a row gives other bytes on at
    least one row, in both orders, so the device-equals-twin comparison on this case would catch that read in the
    kernel."""
    H = D.hessian(case["params"], case["x0"][0])
    assert H.tobytes() != np.ascontiguousarray(H.T).tobytes()
    assert D.tr_transposition_shows(case)


@pytest.mark.skipif(not os.path.isdir(T.REFERENCE), reason="needs the reference tree")
def test_twin_matches_reference_fresh_draw(tmp_path):
    ref = T.reference_solver(T.build_reference(str(tmp_path)))
    rng = np.random.default_rng()
    for n in (2, 5, 16):
        x0 = rng.uniform(-2.5, 2.5, (6, n))
        for stop in ("default", "parity"):
            st = T.make_stop(**T.STOP_PRESETS[stop])
            cfg = T.make_config(initial_radius=float(rng.uniform(0.1, 3.0)))
            assert_same(ref(T.ROSENBROCK, x0, None, st, cfg), T.twin_solve(T.ROSENBROCK, x0, None, st, cfg),
                        "rosenbrock n=%d %s" % (n, stop))
    a = np.concatenate([rng.uniform(-2.0, 3.0, 6), [0.5]])
    x0 = rng.uniform(-2.0, 2.0, (6, 6))
    st = T.make_stop(**{**T.STOP_PRESETS["default"], "num_iterations": 30})
    assert_same(ref(T.DIAG_QUADRATIC, x0, a, st), T.twin_solve(T.DIAG_QUADRATIC, x0, a, st), "diag quadratic")


def test_c_abi_config_defaults():
    from cppnumericalsolvers_amd import capi
    c = capi.default_trust_region_config()
    for k, v in T.DEFAULT_CONFIG.items():
        assert getattr(c, k) == v, k
    assert capi.default_trust_region_config(min_radius=0.5).min_radius == 0.5
    lib = capi.load()
    header = open(os.path.join(T.REPO, "include", "mi355_lbfgs.h")).read()
    declared = sorted(set(re.findall(r"\b(mi355_trust_region_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(capi.TRUST_REGION_SYMBOLS)
    for sym in declared:
        assert hasattr(lib, sym), sym
