"""The stopping-edge table (tests/stop_cases.py) on the CPU: the reference-order twin of TrustRegionNewton, NelderMead,
NewtonDescent, GradientDescent and ConjugatedGradientDescent reproduces every recorded reference solve byte for byte
(NaNs as NaNs), what the generator asserted about the table still holds for the twin of today, and — where the reference
tree exists — the twins equal the freshly built harnesses on a fresh draw under every edge.

The cases with non-default search constants hold inputs only: the reference's constants are constexpr and its harnesses
do not read the config, so there is no reference solve to record for them.  They are checked here for what the twin can
say on its own (the alpha <= alpha_min exit, the two summation orders) and on the device against the twin."""
import os

import numpy as np
import pytest

import fo_lib
import stop_cases as S

CASES = S.load_cases()
RECORDED = [c for c in CASES if "progress" in c]
CONSTANTS = [c for c in CASES if "progress" not in c]
REFERENCE_FIELDS = tuple(k for k in S.PROGRESS_FIELDS if k != "sum_k")      # (the harnesses do not fill sum_k)


def _ids(cases):
    return [c["name"] for c in cases]


def assert_same(ref, twin, what):
    for name, u, v in zip(("x", "f", "g"), ref[:3], twin[:3]):
        assert np.array_equal(u, v, equal_nan=True) and (np.signbit(u) == np.signbit(v)).all(), what + ": " + name
    for k in REFERENCE_FIELDS:
        assert np.array_equal(ref[3][k], twin[3][k], equal_nan=True), what + ": progress." + k


def test_the_table_is_complete():
    names = {c["name"] for c in CASES}
    for key, sv in S.SOLVERS.items():
        for edge in S.EDGE_NAMES:
            assert "%s_rosenbrock_n07_%s" % (key, edge) in names
        assert any(n.startswith(key + "_diag_quadratic_") for n in names)
        assert any(n.startswith("%s_rosenbrock_n%02d_" % (key, sv.spill_n)) for n in names)
        for label, _ in S.CONSTANT_CASES.get(key, ()):
            assert {"%s_rosenbrock_n%02d_%s" % (key, n, label) for n in (7, 9)} <= names
    assert len(CONSTANTS) == 8
    for c in CASES:
        assert int(c["stop"]["num_iterations"][0]) <= S.CAP and 6 <= c["x0"].shape[0] <= 8 and c["x0"].shape[1] <= 12
    assert os.path.getsize(S.GOLDEN) <= os.path.getsize(S.SIZE_CEILING)


@pytest.mark.parametrize("case", RECORDED, ids=_ids(RECORDED))
def test_twin_reference_order_matches_golden(case):
    assert_same((case["x"], case["f"], case["g"], case["progress"]), S.twin_of(case, S.REF_ORDER), case["name"])


@pytest.mark.parametrize("case", RECORDED, ids=_ids(RECORDED))
def test_recorded_case_fires_what_it_targets(case):
    """At least one row ends in the targeted status; only the cases after the limit end on it."""
    p = case["progress"]
    assert np.isin(p["status"], case["target"]).any(), (case["name"], p["status"], case["target"])
    if S.ITERATION_LIMIT not in case["target"]:
        assert (p["status"] != S.ITERATION_LIMIT).all() and (p["num_iterations"] <= S.CAP).all(), case["name"]
    if case["name"].endswith("limit_off"):
        assert int(case["stop"]["num_iterations"][0]) == 0
    if case["name"].endswith("limit1"):
        assert (p["num_iterations"] == 2).all()      # the test is num_iterations > limit (progress.h:212)


@pytest.mark.parametrize("key", list(S.SOLVERS))
@pytest.mark.parametrize("edge", list(S.ONE_STRIKE))
def test_the_strike_count_matters(key, edge):
    """At least one row ends at another iteration than the same solve with one strike."""
    case = next(c for c in CASES if c["name"] == "%s_rosenbrock_n07_%s" % (key, edge))
    one = case["stop"].copy()
    for k, v in S.ONE_STRIKE[edge].items():
        assert int(case["stop"][k][0]) > 1
        one[k] = v
    p1 = S.twin_of(dict(case, stop=one), S.REF_ORDER)[3]
    assert (p1["num_iterations"] != case["progress"]["num_iterations"]).any()


@pytest.mark.parametrize("key,edge", [(k, e) for k in S.SOLVERS for e in S.FLAG_EDGES if (k, e) != ("nm", "grad_abs")])
def test_the_flag_matters(key, edge):
    """The solve with f_delta_relative / gradient_norm_relative flipped ends at another iteration on at least one recorded
    row of the solver: the case tells its flag from the opposite one.  (Nelder-Mead in value mode has no gradient; its
    gradient test fires under neither flag.)"""
    differ, cases = 0, [c for c in RECORDED if c["solver"] == key and c["name"].endswith(edge)]
    assert {int(c["objective"]) for c in cases} >= {S.ROSENBROCK}
    for case in cases:
        other = case["stop"].copy()
        for k, v in S.FLAG_EDGES[edge].items():
            assert int(case["stop"][k][0]) != v
            other[k] = v
        p = S.twin_of(dict(case, stop=other), S.REF_ORDER)[3]
        differ += int((p["num_iterations"] != case["progress"]["num_iterations"]).sum())
    assert differ >= 1


@pytest.mark.parametrize("edge,column,field", [("x_delta_needs_3", 3, "x_delta"), ("f_delta_abs", 4, "f_delta")])
def test_the_reset_branch_is_taken(edge, column, field):
    """A below-threshold delta followed by an above-threshold one before the solve ends (the counter's `else` branch), in
    the trajectory of at least one recorded row (the twins of Nelder-Mead and of the first-order solvers record one)."""
    taken = 0
    for case in RECORDED:
        sv = S.SOLVERS[case["solver"]]
        if not case["name"].endswith(edge) or int(case["objective"]) != S.ROSENBROCK:
            continue
        threshold = float(case["stop"][field][0])
        for row in range(case["x0"].shape[0]):
            rows = sv.twin_trajectory(int(case["objective"]), case["x0"][row], case["params"], case["stop"], case["config"])
            if rows is None:
                continue
            below = rows[:-1, column] < threshold
            above = ~(rows[:, column] < threshold)
            taken += any(below[i] and above[i + 1:].any() for i in range(len(below)))
    assert taken >= 1


def test_marks_are_what_the_twin_says_today():
    marked = []
    for case in CASES:
        ref, dev = S.twin_of(case, S.REF_ORDER), S.twin_of(case, S.DEVICE_ORDER)
        miss = S.misses_contract(ref, dev)
        assert bool(miss.any()) == bool(int(case["marked"])), (case["name"], np.nonzero(miss)[0])
        if int(case["marked"]):
            marked.append(case["name"])
            both = np.isin(ref[3]["status"], S.CONVERGED) & np.isin(dev[3]["status"], S.CONVERGED)
            np.testing.assert_allclose(dev[1][both], ref[1][both], rtol=0, atol=S.CONTRACT, err_msg=case["name"])
    assert len(marked) <= S.MAX_MARKED_FRACTION * len(CASES)
    assert not [m for m in marked if S.never_marked(m)]


def test_constant_cases_reach_their_paths():
    """ConjugatedGradientDescent with alpha_min = 1e-3: at least one search ends on alpha <= alpha_min; no constants case
    runs into the cap; non-default constants change the solve."""
    exits = 0
    for case in CONSTANTS:
        sv = S.SOLVERS[case["solver"]]
        p = S.twin_of(case, S.REF_ORDER)[3]
        assert (p["status"] != S.ITERATION_LIMIT).all(), case["name"]
        default = S.twin_of(dict(case, config=sv.make_config()), S.REF_ORDER)[3]
        assert (default["nfev"] != p["nfev"]).any(), case["name"]
        if case["name"].startswith("cg_") and case["name"].endswith("armijo_a"):
            assert float(case["config"]["alpha_min"][0]) == 1e-3
            cnt = fo_lib.twin_solve(sv.method, int(case["objective"]), case["x0"], case["params"], case["stop"],
                                    case["config"], counters=True)[4]
            exits += int(cnt["alpha_min_exits"].sum())
    assert exits >= 1


def _rosenbrock(x):
    """f, g, H of the chained Rosenbrock function in plain numpy"""
    t = x[1:] - x[:-1] ** 2
    f = np.sum((1.0 - x[:-1]) ** 2 + 100.0 * t ** 2)
    g = np.zeros_like(x)
    g[:-1] = -2.0 * (1.0 - x[:-1]) - 400.0 * x[:-1] * t
    g[1:] += 200.0 * t
    d = np.zeros_like(x)
    d[:-1] = 2.0 - 400.0 * x[1:] + 1200.0 * x[:-1] ** 2
    d[1:] += 200.0
    H = np.diag(d) + np.diag(-400.0 * x[:-1], 1) + np.diag(-400.0 * x[:-1], -1)
    return f, g, H


def test_newton_descent_constants_against_plain_numpy():
    """An independent statement of NewtonDescent with its second-order Armijo search, d = -(H + safe_guard I)^-1 g and
    f(x + alpha d) <= f + alpha (c g.d + c^2/2 d.H d), alpha *= rho: run for as many iterations as the twin took, it
    arrives where the twin did after the same number of trials.  This pins the meaning of safe_guard, armijo_c and
    armijo_rho in the twin (and so on the device) to something written without the twin at hand: with c and rho
    swapped the trial counts differ at once."""
    case = next(c for c in CONSTANTS if c["name"] == "nd_rosenbrock_n07_armijo_a")
    sg, c, rho = (float(case["config"][k][0]) for k in ("safe_guard", "armijo_c", "armijo_rho"))
    assert (sg, c, rho) == (1e-2, 1e-4, 0.5)
    x_twin, _, _, p = S.twin_of(case, S.REF_ORDER)
    assert len(set(p["sum_k"].tolist())) > 1 and (p["sum_k"] > p["num_iterations"]).any()   # some searches shrink alpha
    for row, x in enumerate(case["x0"].copy()):
        trials = 0
        for _ in range(int(p["num_iterations"][row])):
            f, g, H = _rosenbrock(x)
            d = np.linalg.solve(H + sg * np.eye(len(x)), -g)
            slope = c * (g @ d) + 0.5 * c * c * (d @ H @ d)
            alpha, trials = 1.0, trials + 1
            while _rosenbrock(x + alpha * d)[0] > f + alpha * slope:
                alpha, trials = alpha * rho, trials + 1
            x = x + alpha * d
        assert trials == int(p["sum_k"][row]), (row, trials, int(p["sum_k"][row]))
        np.testing.assert_allclose(x, x_twin[row], rtol=0, atol=1e-9)


@pytest.mark.skipif(not os.path.isdir(fo_lib.REFERENCE), reason="needs the reference tree")
@pytest.mark.parametrize("key", list(S.SOLVERS))
def test_twin_matches_reference_fresh_draw(key, tmp_path):
    """Every edge of the solver on a fresh draw of starts against the freshly built harness."""
    sv = S.SOLVERS[key]
    ref = sv.reference(sv.lib.build_reference(str(tmp_path)))
    rng = np.random.default_rng()
    scales = S.TUNING[key]["scales"]
    for n in (7, sv.spill_n):
        x0 = 1.0 + rng.choice(scales, size=(6, 1)) * rng.uniform(-1.0, 1.0, (6, n))
        for edge, (over, _) in S.edges(key).items():
            # (a fresh draw may creep: num_iterations = 0 would not bound it, so the limit-off edge runs under the cap here)
            st = sv.make_stop(**{**over, "num_iterations": over.get("num_iterations") or S.CAP})
            c = sv.make_config()
            if key == "nm" and sv.nm_tied(S.ROSENBROCK, x0, None, st, c).any():
                continue
            assert_same(ref(S.ROSENBROCK, x0, None, st, c), sv.twin(S.ROSENBROCK, x0, None, st, c),
                        "%s n=%d %s" % (key, n, edge))
