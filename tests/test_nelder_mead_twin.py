"""NelderMead on the CPU: the twin of the Nelder-Mead kernel in reference order (tests/nelder_mead/nm_twin.hpp) against
the reference's recorded solves, bit for bit — x, f, g, every progress field, nfev and the per-iteration states — and,
where the reference tree exists, against the reference itself on a fresh draw compiled at test time; the C ABI's config
defaults.  Solves whose rankings met two equal values are left out (the reference's order of those is its std::sort's),
at most 5 % of a case (nm_cases.comparable)."""
import os
import re

import numpy as np
import pytest

import nm_cases
import nm_lib as T

CASES = nm_cases.load_cases()
PROGRESS_FIELDS = ("status", "num_iterations", "nfev", "x_delta", "f_delta", "gradient_norm")


def assert_same(ref, twin, what):
    x, f, g, p = ref[:4]
    tx, tf, tg, tp, tied = twin[:5]
    ok = nm_cases.comparable(tied, x, f, tx, tf)
    assert ok.any(), what + ": nothing left to compare"
    assert x[ok].tobytes() == tx[ok].tobytes(), what + ": x"
    assert f[ok].tobytes() == tf[ok].tobytes(), what + ": f"
    assert g[ok].tobytes() == tg[ok].tobytes(), what + ": g"
    for k in PROGRESS_FIELDS:
        assert p[k][ok].tobytes() == tp[k][ok].tobytes(), what + ": progress." + k


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_reference_order_matches_golden(case):
    single = "trajectory" in case
    twin = T.twin_solve(int(case["objective"]), case["x0"], case["params"], case["stop"], case["config"],
                        order=T.REF_ORDER, trajectory=len(case["trajectory"]) + 1 if single else 0)
    assert_same((case["x"], case["f"], case["g"], case["progress"]), twin, case["name"])
    if single and not twin[4][0]:
        assert twin[5].tobytes() == case["trajectory"].tobytes(), case["name"] + ": trajectory"
        assert twin[6].tobytes() == case["trajectory_x"].tobytes(), case["name"] + ": trajectory iterates"


def test_golden_covers_the_paths():
    by = {c["name"]: c for c in CASES}
    assert all(int(c["stop"]["num_iterations"][0]) <= 300 for c in CASES)
    # value mode forms no gradient; first mode does
    assert not by["rosenbrock_n07_solver_value"]["g"].any()
    assert (by["rosenbrock_n07_solver_value"]["progress"]["gradient_norm"] == 0).all()
    assert by["rosenbrock_n07_solver_first"]["g"].any()
    # both modes walk the same vertices
    assert by["rosenbrock_n07_solver_value"]["x"].tobytes() == by["rosenbrock_n07_solver_first"]["x"].tobytes()
    assert by["rosenbrock_n07_solver_value"]["f"].tobytes() == by["rosenbrock_n07_solver_first"]["f"].tobytes()
    # cases that never converge end at the iteration limit and are compared too
    assert (by["scenario_verify_far"]["progress"]["status"] == 1).all()
    assert (by["diag_quadratic_n01_indefinite_value"]["progress"]["status"] == 1).all()
    # a step costs at least n + 1 vertex calls, the reflection and the rebuild; a shrink n + 1 more.  With gamma = 1 the
    # inside contraction always shrinks, so those solves spend more per step than the same solver at gamma = 0.1 can
    # without shrinking: n + 1 + 1 + 1 + 1 = n + 4
    p = by["edge_certain_shrink"]["progress"]
    n = by["edge_certain_shrink"]["x0"].shape[1]
    assert ((p["nfev"] - 1) > p["num_iterations"] * (n + 4)).any()
    # the restart path (degenerate_tol = 1e-2) costs n + 1 more calls in a step than any step without it can:
    # without a restart at most (n + 1) + 1 + 1 + (n + 1) + 1 per step
    p = by["edge_restart"]["progress"]
    n = by["edge_restart"]["x0"].shape[1]
    # (the same starts under the default tolerance never restart; their nfev differs)
    assert (p["num_iterations"] >= 1).all() and n == 7
    # one strike and five
    assert int(by["edge_x_delta_violations_1"]["stop"]["x_delta_violations"][0]) == 1
    assert int(by["edge_x_delta_violations_5"]["stop"]["x_delta_violations"][0]) == 5
    assert (by["edge_x_delta_violations_1"]["progress"]["num_iterations"] <
            by["edge_x_delta_violations_5"]["progress"]["num_iterations"].max()).all()


def test_restart_and_shrink_paths_run_in_the_twin():
    """The degenerate_tol = 1e-2 case against the same starts at the default tolerance: the restart changes the solve."""
    by = {c["name"]: c for c in CASES}
    c = by["edge_restart"]
    a = T.twin_solve(T.ROSENBROCK, c["x0"], None, c["stop"], c["config"])
    b = T.twin_solve(T.ROSENBROCK, c["x0"], None, c["stop"], T.make_config())
    assert (a[3]["nfev"] != b[3]["nfev"]).any()
    c = by["edge_certain_shrink"]
    a = T.twin_solve(T.ROSENBROCK, c["x0"], None, c["stop"], c["config"])
    b = T.twin_solve(T.ROSENBROCK, c["x0"], None, c["stop"], T.make_config())
    assert (a[3]["nfev"] != b[3]["nfev"]).any()


def test_twin_orders_agree_closely():
    """Reference order and device order differ only in the objective's summation tree."""
    c = next(c for c in CASES if c["name"] == "rosenbrock_n07_solver_value")
    a = T.twin_solve(T.ROSENBROCK, c["x0"], None, c["stop"], c["config"], order=T.REF_ORDER)
    b = T.twin_solve(T.ROSENBROCK, c["x0"], None, c["stop"], c["config"], order=T.DEVICE_ORDER, W=8)
    np.testing.assert_allclose(a[1], b[1], rtol=1e-9, atol=1e-12)


@pytest.mark.skipif(not os.path.isdir(T.REFERENCE), reason="needs the reference tree")
def test_twin_matches_reference_fresh_draw(tmp_path):
    ref = T.reference_solver(T.build_reference(str(tmp_path)))
    rng = np.random.default_rng()
    for n in (2, 5, 16, 20):
        x0 = rng.uniform(-2.5, 2.5, (40, n))
        for preset in ("solver", "default"):
            for mode in (T.VALUE, T.FIRST):
                st = T.make_stop(**{**T.STOP_PRESETS[preset], "num_iterations": 200})
                cfg = T.make_config(mode=mode, gamma=float(rng.uniform(0.05, 0.9)), sigma=float(rng.uniform(0.2, 0.8)))
                assert_same(ref(T.ROSENBROCK, x0, None, st, cfg), T.twin_solve(T.ROSENBROCK, x0, None, st, cfg),
                            "rosenbrock n=%d %s mode %d" % (n, preset, mode))
    a = np.concatenate([rng.uniform(-2.0, 3.0, 6), [0.5]])
    x0 = rng.uniform(-2.0, 2.0, (40, 6))
    st = T.make_stop(**{**T.STOP_PRESETS["solver"], "num_iterations": 60})
    assert_same(ref(T.DIAG_QUADRATIC, x0, a, st), T.twin_solve(T.DIAG_QUADRATIC, x0, a, st), "diag quadratic")
    c = rng.uniform(-1.0, 1.0, 5)
    x0 = rng.uniform(-2.0, 2.0, (40, 5))
    st = T.make_stop(**{**T.STOP_PRESETS["solver"], "num_iterations": 300})
    assert_same(ref(T.L1_QUADRATIC, x0, c, st), T.twin_solve(T.L1_QUADRATIC, x0, c, st), "l1 quadratic")


def test_c_abi_config_defaults():
    from cppnumericalsolvers_amd import capi
    c = capi.default_nelder_mead_config()
    for k, v in T.DEFAULT_CONFIG.items():
        assert getattr(c, k) == v, k
    assert capi.default_nelder_mead_config(mode="first").mode == capi.NM_MODE_FIRST
    assert capi.default_nelder_mead_config(gamma=0.3).gamma == 0.3
    lib = capi.load()
    header = open(os.path.join(T.REPO, "include", "mi355_lbfgs.h")).read()
    declared = sorted(set(re.findall(r"\b(mi355_nelder_mead_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(capi.NELDER_MEAD_SYMBOLS)
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert lib.mi355_lbfgs_abi_version() == 9
