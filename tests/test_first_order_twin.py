"""GradientDescent and ConjugatedGradientDescent on the CPU: the twin of the first-order kernel in reference order
(tests/first_order/fo_twin.hpp) against the reference's recorded solves, bit for bit, per-iteration states included,
and — where the reference tree exists — against the reference itself on a fresh draw compiled at test time; the paths the
recorded cases cover; the device order against the reference order; the C ABI's config defaults."""
import os
import re

import numpy as np
import pytest

import fo_cases
import fo_lib as T

CASES = fo_cases.load_cases()
PROGRESS_FIELDS = ("status", "num_iterations", "nfev", "x_delta", "f_delta", "gradient_norm")


def assert_same(ref, twin, what):
    x, f, g, p = ref
    tx, tf, tg, tp = twin[:4]
    assert x.tobytes() == tx.tobytes(), what + ": x"
    assert f.tobytes() == tf.tobytes(), what + ": f"
    assert g.tobytes() == tg.tobytes(), what + ": g"
    for k in PROGRESS_FIELDS:
        assert p[k].tobytes() == tp[k].tobytes(), what + ": progress." + k


def _twin(case, order, **kw):
    return T.twin_solve(int(case["method"]), int(case["objective"]), case["x0"], case["params"], case["stop"],
                        case["config"], order=order, **kw)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_reference_order_matches_golden(case):
    """x and g against the recorded bytes (n <= 33) or their recorded digests (fo_cases.py); f and every progress field,
    nfev included, against the recorded values."""
    tx, tf, tg, tp = _twin(case, T.REF_ORDER)
    assert fo_cases.same_as_recorded(case, "x", tx), case["name"] + ": x"
    assert fo_cases.same_as_recorded(case, "g", tg), case["name"] + ": g"
    assert case["f"].tobytes() == tf.tobytes(), case["name"] + ": f"
    for k in PROGRESS_FIELDS:
        assert case["progress"][k].tobytes() == tp[k].tobytes(), case["name"] + ": progress." + k


def test_golden_covers_the_paths():
    by = {c["name"]: c for c in CASES}
    assert all(int(c["stop"]["num_iterations"][0]) <= 300 for c in CASES)
    assert os.path.getsize(fo_cases.GOLDEN) <= os.path.getsize(
        os.path.join(os.path.dirname(fo_cases.GOLDEN), "newton_descent_reference_vectors.npz"))
    cnt = {c["name"]: _twin(c, T.REF_ORDER, counters=True)[4] for c in CASES}
    for m in ("gd_", "cg_"):
        assert sum(int(v["alpha_one_steps"].sum()) for k, v in cnt.items() if k.startswith(m)) >= 1
        assert sum(int(v["alpha_less_steps"].sum()) for k, v in cnt.items() if k.startswith(m)) >= 1
    assert sum(int(v["alpha_min_exits"].sum()) for k, v in cnt.items() if k.startswith("cg_")) >= 1
    assert max(int(v["max_trials"].max()) for k, v in cnt.items() if k.startswith("cg_")) == T.MAX_ARMIJO_TRIALS
    assert max(int(c["progress"]["num_iterations"].max()) for c in CASES if c["name"].startswith("cg_")) >= 2
    assert max(int(v["max_trials"].max()) for k, v in cnt.items() if k.startswith("gd_")) >= 3
    assert sum(int(v["refused_searches"].sum()) for k, v in cnt.items() if k.startswith("gd_")) >= 1
    # a start at the minimiser: g = 0, More-Thuente refuses (dginit = -0 >= 0), the step x - g does not move;
    # nfev = 1 + (1 + 1 + 0 trials + 1); ConjugatedGradientDescent: 2 + (1 + 1 + 1 trial + 1)
    p = by["gd_edge_at_minimiser"]["progress"]
    assert (p["x_delta"] == 0).all() and (p["nfev"] == 4).all() and (p["status"] == 2).all()
    p = by["cg_edge_at_minimiser"]["progress"]
    assert (p["x_delta"] == 0).all() and (p["nfev"] == 6).all() and (p["status"] == 2).all()
    # g.g underflows: every GradientDescent step of that case is a refused search (4 steps: 1 + 4 * 3 evaluations)
    assert (by["gd_edge_gg_underflow"]["progress"]["nfev"] == 13).all()
    assert (cnt["gd_edge_gg_underflow"]["refused_searches"] == 4).all()
    # at most a quarter of the cases are marked, none of the scenario / DiagQuadratic ones
    marked = [c["name"] for c in CASES if int(c["marked"])]
    assert len(marked) <= fo_cases.MAX_MARKED_FRACTION * len(CASES)
    assert not [m for m in marked if fo_cases.never_marked(m)]


TRAJECTORY_CASES = [c for c in CASES if "trajectory" in c]


@pytest.mark.parametrize("case", TRAJECTORY_CASES, ids=[c["name"] for c in TRAJECTORY_CASES])
def test_trajectory_matches_recorded_callback_states(case):
    rows, xs = case["trajectory"], case["trajectory_x"]
    assert len(rows) == int(case["progress"]["num_iterations"][0])
    assert (rows[:, 0] == np.arange(1, len(rows) + 1)).all() and (rows[:-1, 1] == 0).all()
    assert rows[-1, 1] == case["progress"]["status"][0]
    assert xs[-1].tobytes() == case["x"][0].tobytes() and rows[-1, 2] == case["f"][0]
    out = T.twin_trajectory(int(case["method"]), int(case["objective"]), case["x0"], case["params"], case["stop"],
                            case["config"], order=T.REF_ORDER, capacity=len(rows) + 1)
    assert out[4].tobytes() == rows.tobytes(), case["name"] + ": the twin's per-iteration records"
    assert out[5].tobytes() == xs.tobytes(), case["name"] + ": the twin's iterates"


@pytest.mark.skipif(not os.path.isdir(T.REFERENCE), reason="needs the reference tree")
def test_twin_matches_reference_fresh_draw(tmp_path):
    lib = T.build_reference(str(tmp_path))
    ref = T.reference_solver(lib)
    rng = np.random.default_rng()
    for method in (T.GRADIENT_DESCENT, T.CONJUGATED_GRADIENT_DESCENT):
        for n in (2, 5, 16, 70):
            x0 = 1.0 + rng.choice((0.05, 0.5, 2.0), size=(6, 1)) * rng.uniform(-1.0, 1.0, (6, n))
            for stop in ("default", "parity"):
                st = T.make_stop(**{**T.STOP_PRESETS[stop], "num_iterations": 120})
                assert_same(ref(method, T.ROSENBROCK, x0, None, st), T.twin_solve(method, T.ROSENBROCK, x0, None, st),
                            "%s rosenbrock n=%d %s" % (T.METHOD_NAMES[method], n, stop))
        a = np.concatenate([rng.uniform(0.5, 3.0, 6), [0.5]])
        x0 = rng.uniform(-2.0, 2.0, (6, 6))
        st = T.make_stop(**{**T.STOP_PRESETS["default"], "num_iterations": 60})
        assert_same(ref(method, T.DIAG_QUADRATIC, x0, a, st), T.twin_solve(method, T.DIAG_QUADRATIC, x0, a, st),
                    T.METHOD_NAMES[method] + " diag quadratic")
        x0 = rng.uniform(-3.0, 3.0, (6, 2))
        assert_same(ref(method, T.QUARTIC, x0, None, st), T.twin_solve(method, T.QUARTIC, x0, None, st),
                    T.METHOD_NAMES[method] + " quartic")
        # the per-iteration states of one start
        x0 = 1.0 + 0.5 * rng.uniform(-1.0, 1.0, (1, 4))
        r = T.reference_trajectory(lib, method, T.ROSENBROCK, x0, None, st)
        t = T.twin_trajectory(method, T.ROSENBROCK, x0, None, st)
        assert r[4].tobytes() == t[4].tobytes() and r[5].tobytes() == t[5].tobytes()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_order_against_reference_order(case):
    """The project's contract between the two summation orders: x* and f* within 1e-6 with equal status.  The generator
    checked it per case and recorded the ones that miss it (fo_cases.py); the record must be what the twin says today."""
    ref = _twin(case, T.REF_ORDER)
    dev = _twin(case, T.DEVICE_ORDER)
    miss = fo_cases.misses_contract(ref, dev)
    assert bool(miss.any()) == bool(int(case["marked"])), (case["name"], np.nonzero(miss)[0])
    if int(case["marked"]):
        both = np.isin(ref[3]["status"], fo_cases.CONVERGED) & np.isin(dev[3]["status"], fo_cases.CONVERGED)
        np.testing.assert_allclose(dev[1][both], ref[1][both], rtol=0, atol=fo_cases.CONTRACT, err_msg=case["name"])


def test_padding_does_not_change_the_device_order():
    """Zeros beyond the padded width add nothing: W x E = 128 and 256 give the bits of 128 at n = 100."""
    case = next(c for c in CASES if c["name"] == "cg_diag_quadratic_n100")
    assert_same(_twin(case, T.DEVICE_ORDER, width=128), _twin(case, T.DEVICE_ORDER, width=256), "width 256")


def test_c_abi_config_defaults():
    from cppnumericalsolvers_amd import capi
    c = capi.default_armijo_config()
    for k, v in T.DEFAULT_CONFIG.items():
        assert getattr(c, k) == v, k
    assert capi.default_armijo_config(rho=0.5).rho == 0.5
    with pytest.raises(TypeError):
        capi.default_armijo_config(safe_guard=1e-5)
    lib = capi.load()
    header = open(os.path.join(T.REPO, "include", "mi355_lbfgs.h")).read()
    declared = sorted(set(re.findall(r"\b(mi355_(?:armijo|gradient_descent|conjugated_gradient_descent)_[a-z0-9_]+)\s*\(",
                                     header)))
    assert declared == sorted(capi.FIRST_ORDER_SYMBOLS)
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert lib.mi355_lbfgs_abi_version() == 9
