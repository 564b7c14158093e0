"""TrustRegionNewton on the MI355X (csrc/trust_region_kernel.hpp): bit for bit the CPU twin in device order on every
recorded case and under two lane mappings, within 1e-6 of the reference's recorded solves with the same status, the
Python driver equal to the host entry point, the dense-Hessian user functor (asymmetric and indefinite Hessians, the
condition test at n up to 64), and clean refusals."""
import ctypes as C

import numpy as np
import pytest

import dense_cases as D
import tr_cases
import tr_lib as T

pytestmark = pytest.mark.gpu
CASES = tr_cases.load_cases()
FIELDS = ("status", "num_iterations", "nfev", "sum_k", "x_delta", "f_delta", "gradient_norm")


def _objective(amd, case):
    obj = int(case["objective"])
    if obj == T.ROSENBROCK:
        return amd.Rosenbrock()
    if obj == T.DIAG_QUADRATIC:
        n = case["x0"].shape[1]
        return amd.DiagQuadratic(case["params"][:n], float(case["params"][n]))
    if obj == T.DENSE:
        return amd.Objective(101, case["params"], "dense_quartic")
    return None


_user_ctx = []


def _context(case):
    """The default library's shared context, or — the dense quartic is a user functor — one on libmi355_lbfgs_tr.so."""
    import cppnumericalsolvers_amd as amd
    if int(case["objective"]) != T.DENSE:
        return None
    if not _user_ctx:
        _user_ctx.append(amd.Context(0, library=_library("libmi355_lbfgs_tr.so")))
    return _user_ctx[0]


def _stop(capi, rec):
    s = capi.Stop()
    for k in T.STOP_DTYPE.names:
        setattr(s, k, rec[k][0].item())
    return s


def _config(rec):
    return {k: rec[k][0].item() for k in T.CONFIG_FIELDS}


def _device_solve(case, lanes=0, trace=None):
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    solver = amd.BatchedTrustRegionNewton(stopping_progress=_stop(capi, case["stop"]), lanes_per_problem=lanes,
                                          condition_hessian=float(case["condition_stop"]), context=_context(case),
                                          **_config(case["config"]))
    x, f, g, p = solver.minimize(_objective(amd, case), torch.from_numpy(case["x0"]).to("cuda:0"), trace=trace)
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


DEVICE_CASES = [c for c in CASES if int(c["objective"]) != T.QUARTIC]


@pytest.mark.parametrize("case", DEVICE_CASES, ids=[c["name"] for c in DEVICE_CASES])
def test_device_matches_twin_and_reference(case):
    n = case["x0"].shape[1]
    W = 8
    while W < n:
        W *= 2
    x, f, g, p = _device_solve(case)
    tx, tf, tg, tp = T.twin_solve(int(case["objective"]), case["x0"], case["params"], case["stop"], case["config"],
                                  float(case["condition_stop"]), order=T.DEVICE_ORDER, W=W)
    assert x.tobytes() == tx.tobytes() and f.tobytes() == tf.tobytes() and g.tobytes() == tg.tobytes(), case["name"]
    for k in FIELDS:
        assert p[k].tobytes() == tp[k].tobytes(), (case["name"], k, p[k], tp[k])
    # against the reference's recorded solve.  The device sums in pairwise trees, the reference in ascending chains: the
    # trajectories part in the last bits, and a LOOSE stop (the default / conservative presets: gradient 1e-5 or 5e-6
    # relative, f plateau over 3 / 5 iterations) then fires a few iterations earlier or later, or the other of the two
    # convergence tests fires first.  The device-order twin shows it on these very inputs: with Rosenbrock n = 32 / 64 under
    # those presets x* moves by up to 5e-4 at f* within 1.1e-7, and 4 of their 32 problems end by the plateau test in one
    # order and by the gradient test in the other; under the parity preset (gradient 1e-8, no plateau) and on every other
    # case x*, f* agree within 1e-7 with the same status.  So: f* within 1e-6 everywhere; status and x* within 1e-6 except
    # on the loose-preset Rosenbrock rows, where both runs must have converged (status 3 or 4) and x* must lie within 1e-3
    # (twice the largest shift the data shows), so that a gross regression still fails there.
    rp = case["progress"]
    if "x" not in case:
        # a dense case above n = 33 keeps a digest of the reference's x*: the twin in reference order, checked against the
        # digest, stands in for it
        case = {**case, "x": D.reference_x(case, T.twin_solve(int(case["objective"]), case["x0"], case["params"],
                                                              case["stop"], case["config"],
                                                              float(case["condition_stop"]))[0])}
    done = rp["status"] != 1     # (an unbounded problem stopped by the iteration limit has no x* to compare)
    # (an overflowing start stays at f = inf in both: equal infinities compare equal here)
    np.testing.assert_allclose(f[done], case["f"][done], rtol=0, atol=1e-6, err_msg=case["name"])
    loose = case["name"].startswith("rosenbrock_n") and not case["name"].endswith("_parity") and n >= 32
    if loose:
        assert np.isin(p["status"], (3, 4)).all() and np.isin(rp["status"], (3, 4)).all(), case["name"]
        np.testing.assert_allclose(x, case["x"], rtol=0, atol=1e-3, err_msg=case["name"])
    else:
        assert (p["status"] == rp["status"]).all(), (case["name"], p["status"], rp["status"])
        np.testing.assert_allclose(x[done], case["x"][done], rtol=0, atol=1e-6, err_msg=case["name"])


@pytest.mark.parametrize("name", ["rosenbrock_n7_default", "rosenbrock_n32_parity", "edge_condition_hessian",
                                  "dense_spd_n09_default", "dense_spd_n33_default"])
def test_lane_mappings_same_bits(name):
    """(The dense case at n = 9 also runs at its padded width of 16 lanes; at n = 33 the padded width is 64.)"""
    case = next(c for c in CASES if c["name"] == name)
    a = _device_solve(case)
    b = _device_solve(case, lanes=64)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes(), name
    if name == "dense_spd_n09_default":
        for u, v in zip(a, _device_solve(case, lanes=16)):
            assert u.tobytes() == v.tobytes(), name + " (16 lanes)"


def test_python_driver_equals_host_entry():
    import cppnumericalsolvers_amd as amd
    case = next(c for c in CASES if c["name"] == "rosenbrock_n32_default")
    x, f, g, p = _device_solve(case)
    from cppnumericalsolvers_amd import capi
    solver = amd.BatchedTrustRegionNewton(stopping_progress=_stop(capi, case["stop"]), **_config(case["config"]))
    hx, hf, hg, hp = solver.minimize_host(amd.Rosenbrock(), case["x0"])
    assert x.tobytes() == hx.tobytes() and f.tobytes() == hf.tobytes() and g.tobytes() == hg.tobytes()
    assert p.tobytes() == hp.tobytes()


def test_refusals_are_clean_errors():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    x65 = torch.zeros((2, 65), dtype=torch.float64, device="cuda:0")
    with pytest.raises(Exception, match="n <= 64"):
        amd.BatchedTrustRegionNewton().minimize(amd.Rosenbrock(), x65)
    x4 = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    solver = amd.BatchedTrustRegionNewton()
    solver.arithmetic = capi.ARITH_FMA
    with pytest.raises(Exception, match="exact arithmetic"):
        solver.minimize(amd.Rosenbrock(), x4)
    A = np.ones((3, 4))
    y = np.zeros((2, 3))
    with pytest.raises(Exception, match="device Hessian"):
        amd.BatchedTrustRegionNewton().minimize(amd.SquaredErrorRidge(A, 0.1), x4,
                                                per_problem=torch.from_numpy(y).to("cuda:0"))


def test_reference_scenarios_over_the_drop_in_header():
    """tests/trust_region/tr_header_test.cc: the reference's trust-region scenarios with its own bounds, callbacks
    included, through include/cppoptlib/solver/trust_region_newton.h (built by build())."""
    import os
    import subprocess
    exe = os.path.join(T.TR_DIR, "_build", "tr_header_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def _library(name):
    import os
    return os.path.join(T.REPO, "cppnumericalsolvers_amd", name)


def _quartic_solve(case, trace=None):
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    ctx = amd.Context(0, library=_library("libmi355_lbfgs_tr.so"))
    solver = amd.BatchedTrustRegionNewton(stopping_progress=_stop(capi, case["stop"]), context=ctx,
                                          **_config(case["config"]))
    x, f, g, p = solver.minimize(amd.Objective(100, np.zeros(0), "quartic"), torch.from_numpy(case["x0"]).to("cuda:0"),
                                 trace=trace)
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


QUARTIC_CASES = [c for c in CASES if int(c["objective"]) == T.QUARTIC]


@pytest.mark.parametrize("case", QUARTIC_CASES, ids=[c["name"] for c in QUARTIC_CASES])
def test_user_functor_quartic(case):
    """The quartic double well as a user device functor (examples/user_objective_quartic, libmi355_lbfgs_tr.so): bit for
    bit the device-order twin, within 1e-6 of the reference with the same status."""
    x, f, g, p = _quartic_solve(case)
    tx, tf, tg, tp = T.twin_solve(T.QUARTIC, case["x0"], None, case["stop"], case["config"], order=T.DEVICE_ORDER, W=8)
    assert x.tobytes() == tx.tobytes() and f.tobytes() == tf.tobytes() and g.tobytes() == tg.tobytes()
    for k in FIELDS:
        assert p[k].tobytes() == tp[k].tobytes(), k
    assert (p["status"] == case["progress"]["status"]).all()
    np.testing.assert_allclose(x, case["x"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(f, case["f"], rtol=0, atol=1e-6)


def test_quartic_double_well_scenario_reference_bounds():
    """QuarticDoubleWellConvergesDespiteDegenerateStart of trust_region_newton_test.cc on the device: x0 = 0.1,
    initial_radius 0.5, gradient_norm 1e-10, 100 iterations; |x*| within 1e-6 of sqrt(2) in fewer than 50 iterations."""
    case = next(c for c in CASES if c["name"] == "scenario_quartic_double_well")
    assert case["config"]["initial_radius"][0] == 0.5 and case["stop"]["gradient_norm"][0] == 1e-10
    x, f, g, p = _quartic_solve(case)
    assert abs(abs(x[0, 0]) - np.sqrt(2.0)) <= 1e-6
    assert p["num_iterations"][0] < 50


TRAJECTORY_CASES = [c for c in CASES if "trajectory" in c]


@pytest.mark.parametrize("case", TRAJECTORY_CASES, ids=[c["name"] for c in TRAJECTORY_CASES])
def test_trajectory_matches_reference_callback(case):
    """The per-iteration states the device traces (what the callback replay hands a user) against the states the
    reference's own step callback saw: the same number of iterations, the same status at every one, value, x_delta,
    f_delta, gradient_norm and the iterate within 1e-6."""
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    n = case["x0"].shape[1]
    trace = amd.Trace([0], capacity=1024, n=n, device=torch.device("cuda", 0), with_x=True)
    if int(case["objective"]) == T.QUARTIC:
        _quartic_solve(case, trace=trace)
    elif int(case["objective"]) == T.DENSE:
        _device_solve(case, trace=trace)
    else:
        solver = amd.BatchedTrustRegionNewton(stopping_progress=_stop(capi, case["stop"]),
                                              condition_hessian=float(case["condition_stop"]), **_config(case["config"]))
        solver.minimize(_objective(amd, case), torch.from_numpy(case["x0"]).to("cuda:0"), trace=trace)
        torch.cuda.synchronize()
    rec, xs, _ = trace.history(0)
    ref, ref_x = case["trajectory"], case["trajectory_x"]
    assert len(rec) == len(ref), (case["name"], len(rec), len(ref))
    assert (rec["num_iterations"] == ref[:, 0]).all()
    assert (rec["status"] == ref[:, 1]).all(), (case["name"], rec["status"], ref[:, 1])
    for col, k in enumerate(("value", "x_delta", "f_delta", "gradient_norm"), start=2):
        np.testing.assert_allclose(rec[k], ref[:, col], rtol=0, atol=1e-6, err_msg="%s %s" % (case["name"], k))
    np.testing.assert_allclose(xs, ref_x, rtol=0, atol=1e-6, err_msg=case["name"])


def test_library_without_trust_region_kernels_refuses():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    ctx = amd.Context(0, library=_library("libmi355_lbfgs_svm.so"))   # user objective 100 built for Lbfgs only
    x0 = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.EngineError) as e:
        amd.BatchedTrustRegionNewton(context=ctx).minimize(amd.Objective(100, np.zeros(1), "svm"), x0)
    assert e.value.code == capi.ERR_UNSUPPORTED
    # (capi.check reads the text from the first loaded library that holds one: ask the failing library itself)
    assert b"no trust-region kernel" in ctx._lib.mi355_lbfgs_last_error()
