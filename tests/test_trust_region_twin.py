"""TrustRegionNewton on the CPU: the twin of the trust-region kernel in reference order (tests/trust_region/tr_twin.hpp)
against the reference's recorded solves, bit for bit, and — where the reference tree exists — against the reference
itself on a fresh draw compiled at test time; the C ABI's config defaults."""
import os
import re

import numpy as np
import pytest

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
