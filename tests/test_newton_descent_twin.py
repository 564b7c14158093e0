"""NewtonDescent on the CPU: the twin of the Newton-descent kernel in reference order
(tests/newton_descent/nd_twin.hpp) against the reference's recorded solves, bit for bit, per-iteration states included,
and — where the reference tree exists — against the reference itself on a fresh draw compiled at test time; the bound of
the search; the device order against the reference order; the C ABI's config defaults."""
import os
import re

import numpy as np
import pytest

import dense_cases as D
import nd_cases
import nd_lib as T

CASES = nd_cases.load_cases()
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
    return T.twin_solve(int(case["objective"]), case["x0"], case["params"], case["stop"], case["config"],
                        float(case["condition_stop"]), order=order, **kw)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_reference_order_matches_golden(case):
    twin = _twin(case, T.REF_ORDER, counters=True)
    assert (twin[4]["fixed_point"] == 0).all()    # (a solve that got there is not comparable with the reference)
    if "g" not in case:
        # a dense case: g* (and x* above n = 33) recorded as digests of the reference's bytes (dense_cases.py)
        assert D.same_as_recorded(case, "x", twin[0]), case["name"] + ": x"
        assert D.same_as_recorded(case, "g", twin[2]), case["name"] + ": g"
        case = {**case, "x": twin[0], "g": twin[2]}
    assert_same((case["x"], case["f"], case["g"], case["progress"]), twin, case["name"])


def test_golden_covers_the_paths():
    by = {c["name"]: c for c in CASES}
    assert all(int(c["stop"]["num_iterations"][0]) <= 300 for c in CASES)
    cnt = {c["name"]: _twin(c, T.REF_ORDER, counters=True)[4] for c in CASES}
    assert sum(int(v["interchanges"].sum()) for v in cnt.values()) >= 1
    assert max(int(v["max_trials"].max()) for v in cnt.values()) >= 100
    assert sum(int(v["alpha_one_steps"].sum()) for v in cnt.values()) >= 1
    assert sum(int(v["alpha_less_steps"].sum()) for v in cnt.values()) >= 1
    # a start at the minimiser: d = 0, alpha = 1, x_delta = 0; nfev = 1 + (1 + 1 + 1 trial + 1)
    p = by["edge_at_minimiser"]["progress"]
    assert (p["x_delta"] == 0).all() and (p["nfev"] == 5).all() and (p["status"] == 2).all()
    # the stall: some search ran out of resolution and the x_delta test ended the solve
    assert (by["rosenbrock_n08_stall"]["progress"]["status"] == 2).any()
    assert (by["edge_condition_hessian"]["progress"]["status"] == 5).any()
    # at most a quarter of the cases are marked, none of the scenario / DiagQuadratic / quartic ones
    marked = [c["name"] for c in CASES if int(c["marked"])]
    assert len(marked) <= nd_cases.MAX_MARKED_FRACTION * len(CASES)
    assert not [m for m in marked if m.startswith(nd_cases.NEVER_MARKED)]


def test_dense_cases_reach_the_lu_and_the_condition_test():
    """What the generator asserted of the dense-Hessian cases, from the twin's counters today: far pivots at n >= 33 (past
    the 8-wide chunks of the device's search and past 32 rows), pivots beyond the neighbouring row on both sides of the
    n = 8 boundary, exact ties, both step kinds, condition numbers away from the threshold with both decisions taken, and
    an all-zero pivot column in the device-only edge case."""
    by = {c["name"]: c for c in CASES}
    cnt = {nm: _twin(c, T.REF_ORDER, counters=True)[4] for nm, c in by.items() if nm.startswith("dense_")}
    assert sorted(int(nm[11:13]) for nm in cnt if nm.startswith("dense_spd_") and nm.endswith("_default")) == list(D.DIMS)
    for n in D.DIMS:
        for kind in ("dense_spd_n%02d_default", "dense_spd_n%02d_parity", "dense_asym_n%02d_default"):
            assert by[kind % n]["x0"].shape == (8, n)
        h = cnt["dense_spd_n%02d_default" % n]["pivot_distance"].sum(axis=0)
        if n >= 33:
            assert h[8:].sum() >= 100 and h[32:].sum() >= 10, (n, h[8:].sum(), h[32:].sum())
        if n in (8, 9):
            assert h[2:].sum() >= 10, (n, h[2:].sum())
    assert any(cnt["dense_spd_n%02d_default" % n]["pivot_ties"].sum() >= 1 for n in D.DIMS if n >= 9)
    assert sum(int(v["alpha_one_steps"].sum()) for v in cnt.values()) >= 1
    assert sum(int(v["alpha_less_steps"].sum()) for v in cnt.values()) >= 1
    for n in (9, 33, 64):
        name = "dense_condition_n%02d" % n
        status = by[name]["progress"]["status"]
        margin = min(cnt[name]["min_condition_margin"].min(),
                     _twin(by[name], T.DEVICE_ORDER, counters=True)[4]["min_condition_margin"].min())
        assert margin >= 1e-9, name      # (every condition number either order evaluates)
        assert (status == 5).any() and (status != 5).any(), (name, status)
        assert (by[name]["progress"]["num_iterations"][status == 5] >= 2).any(), name
    z = D.zero_column_case()
    zc = T.twin_solve(D.DENSE, z["x0"], z["params"], z["stop"], z["config"], 0.0, counters=True)[4]
    assert (zc["zero_columns"] >= 1).all() and (zc["fixed_point"] == 0).all()


ASYMMETRIC_CASES = [c for c in CASES if c["name"].startswith("dense_asym_")]


@pytest.mark.parametrize("case", ASYMMETRIC_CASES, ids=[c["name"] for c in ASYMMETRIC_CASES])
def test_asymmetric_cases_notice_a_transposed_hessian(case):
    """H(i, j) != H(j, i) in the last bits: the twin with H transposed before the LU gives other bytes on at least one
    row, in both orders, so the device-equals-twin comparison on this case would catch that read in the kernel.  (The
    chain of the search: test_strongly_asymmetric_cases_notice_a_chain_walking_a_row.)"""
    H = D.hessian(case["params"], case["x0"][0])
    assert H.tobytes() != np.ascontiguousarray(H.T).tobytes()
    assert D.nd_transposition_shows(case)


@pytest.mark.parametrize("n", sorted(D.CHAIN_CASES))
def test_strongly_asymmetric_cases_notice_a_chain_walking_a_row(n):
    """dense_cases.chain_case: S with an antisymmetric part of 2^60 and more.  The twin whose search walks row j of H for
    column j in v_j = sum_i (k d_i) H(i, j) gives other bytes on at least one row, in both orders, so the
    device-equals-twin comparison on this case (tests/test_gpu_newton_descent.py) holds the kernel's column walk to
    its comment: it does not rely on a symmetric H."""
    case = D.chain_case(n)
    assert D.nd_mutation_shows(T.CHAIN_WALKS_ROW, case)
    out = _twin(case, T.DEVICE_ORDER, counters=True)
    assert np.isfinite(out[0]).all() and (out[4]["alpha_less_steps"] >= 1).any()


def test_dense_kappa0_lands_on_the_linear_solve():
    """kappa = 0: H = S is constant and every step is a full Newton step on (S + 1e-5 I), which leaves 1e-5 / lambda_min
    of the error behind; under the parity stop three of them end the solve.  x* against S x = b solved with 50 digits,
    to 1e-6."""
    import mpmath
    case = next(c for c in CASES if c["name"] == "dense_kappa0_n17")
    n = case["x0"].shape[1]
    p = case["params"]
    assert p[n * n + n] == 0.0 and (case["progress"]["num_iterations"] <= 3).all()
    assert (_twin(case, T.REF_ORDER, counters=True)[4]["alpha_less_steps"] == 0).all()
    with mpmath.workdps(50):
        S = mpmath.matrix(p[:n * n].reshape(n, n).T.tolist())
        exact = np.array([float(v) for v in mpmath.lu_solve(S, mpmath.matrix(p[n * n:n * n + n].tolist()))])
    np.testing.assert_allclose(case["x"], np.tile(exact, (case["x0"].shape[0], 1)), rtol=0, atol=1e-6)


TRAJECTORY_CASES = [c for c in CASES if "trajectory" in c]


@pytest.mark.parametrize("case", TRAJECTORY_CASES, ids=[c["name"] for c in TRAJECTORY_CASES])
def test_reference_callback_states_end_at_the_result(case):
    rows, xs = case["trajectory"], case["trajectory_x"]
    assert len(rows) == int(case["progress"]["num_iterations"][0])
    assert (rows[:, 0] == np.arange(1, len(rows) + 1)).all() and (rows[:-1, 1] == 0).all()
    assert rows[-1, 1] == case["progress"]["status"][0]
    assert xs[-1].tobytes() == case["x"][0].tobytes() and rows[-1, 2] == case["f"][0]
    for col, k in ((3, "x_delta"), (4, "f_delta"), (5, "gradient_norm")):
        assert rows[-1, col] == case["progress"][k][0]


@pytest.mark.skipif(not os.path.isdir(T.REFERENCE), reason="needs the reference tree")
def test_twin_matches_reference_fresh_draw(tmp_path):
    lib = T.build_reference(str(tmp_path))
    ref = T.reference_solver(lib)
    rng = np.random.default_rng()

    def comparable(objective, x0, params, st):
        twin = T.twin_solve(objective, x0, params, st, counters=True)
        keep = twin[4]["fixed_point"] == 0
        assert keep.any()
        return np.ascontiguousarray(x0[keep])
    for n in (2, 5, 16):
        x0 = 1.0 + rng.choice((0.05, 0.5, 2.0), size=(6, 1)) * rng.uniform(-1.0, 1.0, (6, n))
        for stop in ("default", "parity"):
            st = T.make_stop(**{**T.STOP_PRESETS[stop], "num_iterations": 200})
            x0c = comparable(T.ROSENBROCK, x0, None, st)
            assert_same(ref(T.ROSENBROCK, x0c, None, st), T.twin_solve(T.ROSENBROCK, x0c, None, st),
                        "rosenbrock n=%d %s" % (n, stop))
    a = np.concatenate([rng.uniform(-2.0, 3.0, 6), [0.5]])
    x0 = rng.uniform(-2.0, 2.0, (6, 6))
    st = T.make_stop(**{**T.STOP_PRESETS["default"], "num_iterations": 30})
    x0c = comparable(T.DIAG_QUADRATIC, x0, a, st)
    assert_same(ref(T.DIAG_QUADRATIC, x0c, a, st), T.twin_solve(T.DIAG_QUADRATIC, x0c, a, st), "diag quadratic")
    x0 = rng.uniform(-3.0, 3.0, (6, 2))
    x0c = comparable(T.QUARTIC, x0, None, st)
    assert_same(ref(T.QUARTIC, x0c, None, st), T.twin_solve(T.QUARTIC, x0c, None, st), "quartic")
    # the per-iteration states: one start, the twin's solve ends where the callback's last state is
    x0 = 1.0 + 0.5 * rng.uniform(-1.0, 1.0, (1, 4))
    st = T.make_stop(**{**T.STOP_PRESETS["default"], "num_iterations": 200})
    if len(comparable(T.ROSENBROCK, x0, None, st)):
        x, f, g, p, rows, xs = T.reference_trajectory(lib, T.ROSENBROCK, x0, None, st)
        tx, tf, tg, tp = T.twin_solve(T.ROSENBROCK, x0, None, st)
        assert xs[-1].tobytes() == tx[0].tobytes() and rows[-1, 2] == tf[0] and len(rows) == tp["num_iterations"][0]


def test_search_is_bounded_at_the_fixed_point_of_alpha():
    """d = +inf on the quartic double well at x = 0.1 (g < 0, H < 0): the trial value is +inf, the Armijo bound -inf at
    every alpha, so the reference's loop never ends.  The twin's (and the kernel's) ends where alpha * rho == alpha."""
    a, shrinks = 1.0, 0
    while a * 0.9 != a:
        a *= 0.9
        shrinks += 1
    assert shrinks == T.FIXED_POINT_SHRINKS and a == 2.5e-323
    for order in (T.REF_ORDER, T.DEVICE_ORDER):
        alpha, trials, fixed = T.twin_search(T.QUARTIC, np.array([0.1]), np.array([np.inf]), order=order)
        assert fixed and alpha == a
        assert trials - 1 <= T.FIXED_POINT_SHRINKS
    # an ordinary search does not get there
    alpha, trials, fixed = T.twin_search(T.ROSENBROCK, np.array([-1.2, 1.0]), np.array([1.0, 1.0]))
    assert not fixed and trials < 400


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_order_against_reference_order(case):
    """The project's contract between the two summation orders: x* and f* within 1e-6 with equal status.  The generator
    checked it per case and recorded the ones that miss it (nd_cases.py); the record must be what the twin says today."""
    ref = _twin(case, T.REF_ORDER)
    dev = _twin(case, T.DEVICE_ORDER)
    miss = nd_cases.misses_contract(ref, dev)
    assert bool(miss.any()) == bool(int(case["marked"])), (case["name"], np.nonzero(miss)[0])
    if int(case["marked"]):
        both = np.isin(ref[3]["status"], nd_cases.CONVERGED) & np.isin(dev[3]["status"], nd_cases.CONVERGED)
        np.testing.assert_allclose(dev[1][both], ref[1][both], rtol=0, atol=nd_cases.CONTRACT, err_msg=case["name"])


def test_lane_width_does_not_change_the_lu_or_the_solve():
    """No reductions in the LU and the solve: on a problem whose objective has no sum (the quartic) every width gives
    the bits of the reference order."""
    case = next(c for c in CASES if c["name"] == "quartic_n03")
    ref = _twin(case, T.REF_ORDER)
    for W in (8, 16, 32, 64):
        assert_same(ref, _twin(case, T.DEVICE_ORDER, W=W), "W=%d" % W)


def test_c_abi_config_defaults():
    from cppnumericalsolvers_amd import capi
    c = capi.default_newton_descent_config()
    for k, v in T.DEFAULT_CONFIG.items():
        assert getattr(c, k) == v, k
    assert capi.default_newton_descent_config(armijo_rho=0.5).armijo_rho == 0.5
    with pytest.raises(TypeError):
        capi.default_newton_descent_config(alpha_min=1e-8)
    lib = capi.load()
    header = open(os.path.join(T.REPO, "include", "mi355_lbfgs.h")).read()
    declared = sorted(set(re.findall(r"\b(mi355_newton_descent_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(capi.NEWTON_DESCENT_SYMBOLS)
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert lib.mi355_lbfgs_abi_version() == 9
