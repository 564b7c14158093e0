"""progress_stop_tests (csrc/progress_device.hpp) on the MI355X through the four kernels that call it: TrustRegionNewton,
NelderMead, NewtonDescent, and the first-order kernel as GradientDescent and as ConjugatedGradientDescent.

1. Every recorded stopping-edge case (tests/stop_cases.py): bit for bit the device-order twin; on unmarked cases the
   reference's status, and f and x within 1e-6 of the recorded solve; on marked cases f within 1e-6 where both converged.
2. Traced statuses of one strike case and one plateau case per solver: CONTINUE up to the last record, as many records
   as the reference took iterations.
3. Re-fetch with live counters, once per kernel (GradientDescent and ConjugatedGradientDescent apart): 600 mixed
   Rosenbrock-8 rows through a grid capped at 2 workgroups under x_delta with 3 strikes, f_delta with 2 strikes and a
   ring of 8, so that a segment fetches its next problem with non-zero counters and a full ring.  (With the counters'
   reset at fetch taken out of the device-order twin, 9 / 431 / 11 / 166 / 163 of the 600 rows of tr / nm / nd / gd / cg
   change when one segment serves the queue in order: the batches tell a stale counter from a fresh one.)
4. Non-default search constants of NewtonDescent and ConjugatedGradientDescent: bit for bit the device-order twin (the
   reference's constants are constexpr, so there is no recorded solve; unmarked cases are held to the 1e-6 contract
   against the twin in reference order, which tests/test_stopping_edges_twin.py pins to the reference under the default
   constants).  The eval_trials path of the ConjugatedGradientDescent kernel: the bytes of the default context."""
import numpy as np
import pytest

import fo_cases
import fo_lib
import stop_cases as S
import tr_queue as Q

pytestmark = pytest.mark.gpu
CASES = S.load_cases()
BY_NAME = {c["name"]: c for c in CASES}
RECORDED = [c for c in CASES if "progress" in c]
CONSTANTS = [c for c in CASES if "progress" not in c]
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
EVAL_TRIALS_ENV = "MI355_DEBUG_CG_EVAL_TRIALS"


def _objective(amd, objective, n, params):
    if objective == S.ROSENBROCK:
        return amd.Rosenbrock()
    return amd.DiagQuadratic(params[:n], float(params[n]))


def _stop(rec):
    from cppnumericalsolvers_amd import capi
    s = capi.Stop()
    for k in fo_lib.STOP_DTYPE.names:
        setattr(s, k, rec[k][0].item())
    return s


def _solver(key, stop, config, context=None):
    import cppnumericalsolvers_amd as amd
    fields = S.SOLVERS[key].lib.CONFIG_FIELDS
    kw = {k: config[k][0].item() for k in fields}
    if key == "tr":
        return amd.BatchedTrustRegionNewton(stopping_progress=_stop(stop), context=context, **kw)
    if key == "nm":
        return amd.BatchedNelderMead(stopping_progress=_stop(stop), context=context, **kw)
    if key == "nd":
        return amd.BatchedNewtonDescent(stopping_progress=_stop(stop), context=context, **kw)
    if key == "gd":
        return amd.BatchedGradientDescent(stopping_progress=_stop(stop), context=context)
    return amd.BatchedConjugatedGradientDescent(stopping_progress=_stop(stop), context=context,
                                                **{"armijo_" + k: v for k, v in kw.items()})


def _run(solver, objective, x0, trace=None):
    import torch
    import cppnumericalsolvers_amd as amd
    x, f, g, p = solver.minimize(objective, torch.from_numpy(np.ascontiguousarray(x0)).to("cuda:0"), trace=trace)
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


def _device_solve(case, trace=None, context=None):
    import cppnumericalsolvers_amd as amd
    n = case["x0"].shape[1]
    solver = _solver(case["solver"], case["stop"], case["config"], context)
    return _run(solver, _objective(amd, int(case["objective"]), n, case["params"]), case["x0"], trace)


def _assert_same_bits(a, b, what):
    diff = Q.same_bits(a, b)
    assert diff is None, "%s: %s" % (what, diff)


@pytest.mark.parametrize("case", RECORDED, ids=[c["name"] for c in RECORDED])
def test_device_matches_twin_and_reference(case):
    out = _device_solve(case)
    _assert_same_bits(out, S.twin_of(case, S.DEVICE_ORDER), case["name"])
    x, f, g, p = out
    rp = case["progress"]
    print(case["name"], "status", p["status"].tolist(), "reference", rp["status"].tolist(), "max|df| %.3g max|dx| %.3g"
          % (np.max(np.abs(f - case["f"])), np.max(np.abs(x - case["x"]))))
    if int(case["marked"]):
        both = np.isin(p["status"], S.CONVERGED) & np.isin(rp["status"], S.CONVERGED)
        np.testing.assert_allclose(f[both], case["f"][both], rtol=0, atol=1e-6, err_msg=case["name"])
        return
    assert (p["status"] == rp["status"]).all(), (case["name"], p["status"], rp["status"])
    np.testing.assert_allclose(f, case["f"], rtol=0, atol=1e-6, err_msg=case["name"])
    np.testing.assert_allclose(x, case["x"], rtol=0, atol=1e-6, err_msg=case["name"])


@pytest.mark.parametrize("case", CONSTANTS, ids=[c["name"] for c in CONSTANTS])
def test_non_default_search_constants(case):
    out = _device_solve(case)
    _assert_same_bits(out, S.twin_of(case, S.DEVICE_ORDER), case["name"])
    if not int(case["marked"]):
        ref = S.twin_of(case, S.REF_ORDER)
        assert not S.misses_contract(out, ref).any(), case["name"]


TRACED = ["%s_rosenbrock_n07_%s" % (key, edge) for key in S.SOLVERS for edge in S.TRACED_EDGES]


@pytest.mark.parametrize("name", TRACED)
def test_traced_statuses(name):
    """Row 0 of a strike case and of a plateau case: every traced status but the last is CONTINUE, the last is the
    recorded one, and there are as many records as the reference took iterations."""
    import torch
    import cppnumericalsolvers_amd as amd
    case = BY_NAME[name]
    assert not int(case["marked"])
    n = case["x0"].shape[1]
    trace = amd.Trace([0], capacity=S.CAP + 2, n=n, device=torch.device("cuda", 0), with_x=False)
    _device_solve(case, trace=trace)
    rec = trace.history(0)[0]
    rp = case["progress"]
    assert len(rec) == int(rp["num_iterations"][0]), (name, len(rec), int(rp["num_iterations"][0]))
    assert (rec["num_iterations"] == np.arange(1, len(rec) + 1)).all()
    assert (rec["status"][:-1] == S.CONTINUE).all(), (name, rec["status"])
    assert rec["status"][-1] == rp["status"][0] and rp["status"][0] in case["target"], (name, rec["status"][-1])


@pytest.mark.parametrize("key", list(S.SOLVERS))
def test_refetch_with_live_counters(key, monkeypatch, gpu_solver_factory):
    """(gpu_solver_factory is asked for first, so that the session's shared context is never created under the cap.)"""
    import cppnumericalsolvers_amd as amd
    sv = S.SOLVERS[key]
    n, B, cap = 8, 600, 2
    x0 = Q.mixed_rosenbrock_batch(n, B, S.CAPPED_SEED)[0]
    stop, config = S.capped_stop(key), sv.make_config()
    assert int(stop["x_delta_violations"][0]) == 3 and int(stop["f_delta_violations"][0]) == 2
    assert float(stop["f_delta"][0]) > 0 and int(stop["past"][0]) == 8 and int(stop["num_iterations"][0]) == 40
    twin = sv.twin_threaded(S.ROSENBROCK, x0, None, stop, config, order=S.DEVICE_ORDER, W=8)
    st = twin[3]["status"]
    assert (st == S.X_DELTA).any() and (st == S.F_DELTA).any(), np.unique(st, return_counts=True)
    assert len(set(twin[3]["num_iterations"].tolist())) > 3
    monkeypatch.setenv(CAP_ENV, str(cap))
    ctx = amd.Context(0)
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        solver = _solver(key, stop, config, context=ctx)
        out = _run(solver, amd.Rosenbrock(), x0)
        ll = solver.last_launch()
        assert ll["blocks"] == cap and ll["lanes_per_problem"] == 8, ll
    finally:
        ctx.close()
    _assert_same_bits(out, twin, key + " capped grid")


FO_CASES = {c["name"]: c for c in fo_cases.load_cases()}


@pytest.mark.parametrize("name", ["cg_rosenbrock_n007_default", "cg_diag_quadratic_n005", "cg_diag_quadratic_n100"])
def test_eval_trials_path_returns_the_same_bytes(name, monkeypatch, gpu_solver_factory):
    """A context created with MI355_DEBUG_CG_EVAL_TRIALS=1 runs eval at the Armijo trial points and keeps the last
    gradient: the bytes of the default context, nfev and sum_k included (n = 100 is the 64 x 2 mapping)."""
    import cppnumericalsolvers_amd as amd
    case = FO_CASES[name]
    n = case["x0"].shape[1]
    objective = _objective(amd, int(case["objective"]), n, case["params"])
    base_solver = _solver("cg", case["stop"], case["config"])
    base = _run(base_solver, objective, case["x0"])
    monkeypatch.setenv(EVAL_TRIALS_ENV, "1")
    ctx = amd.Context(0)
    monkeypatch.delenv(EVAL_TRIALS_ENV, raising=False)
    try:
        solver = _solver("cg", case["stop"], case["config"], context=ctx)
        out = _run(solver, objective, case["x0"])
        ll = solver.last_launch()
    finally:
        ctx.close()
    if n == 100:
        assert ll["lanes_per_problem"] == 64 and ll["elems_per_lane"] == 2, ll
    _assert_same_bits(out, base, name + " eval_trials")
    assert (out[3]["sum_k"] > 0).all()
    _assert_same_bits(out, fo_lib.twin_solve(fo_lib.CONJUGATED_GRADIENT_DESCENT, int(case["objective"]), case["x0"],
                                             case["params"], case["stop"], case["config"], order=fo_lib.DEVICE_ORDER),
                      name + " twin")
