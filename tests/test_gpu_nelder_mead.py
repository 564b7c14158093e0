"""NelderMead on the MI355X (csrc/nelder_mead_kernel.hpp): bit for bit the CPU twin in device order on every recorded
case through every lane mapping that covers n (n = W, where the n + 1 vertices exceed the segment, and n = W + 1
included), value mode and first mode agreeing on the walk, the device trace against the reference's per-iteration
states, the verify.cc scenarios through the drop-in header, the value-only l1 example library, clean refusals, and a batch
larger than a capped resident grid."""
import os
import subprocess

import numpy as np
import pytest

import nm_cases
import nm_lib as T

pytestmark = pytest.mark.gpu
CASES = nm_cases.load_cases()
BY_NAME = {c["name"]: c for c in CASES}
FIELDS = ("status", "num_iterations", "nfev", "sum_k", "x_delta", "f_delta", "gradient_norm")
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"


def _objective(amd, case):
    obj = int(case["objective"])
    n = case["x0"].shape[1]
    if obj == T.ROSENBROCK:
        return amd.Rosenbrock()
    if obj == T.DIAG_QUADRATIC:
        return amd.DiagQuadratic(case["params"][:n], float(case["params"][n]))
    return amd.Objective(100, np.asarray(case["params"][:n], dtype=np.float64), "l1_quadratic")


def _stop(capi, rec, **over):
    s = capi.Stop()
    for k in T.STOP_DTYPE.names:
        setattr(s, k, rec[k][0].item())
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _config(rec, **over):
    return {**{k: rec[k][0].item() for k in T.CONFIG_FIELDS}, **over}


def _device_solve(case, lanes=0, context=None, trace=None, stop_over=None, config_over=None, x0=None):
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    solver = amd.BatchedNelderMead(stopping_progress=_stop(capi, case["stop"], **(stop_over or {})), context=context,
                                   lanes_per_problem=lanes, **_config(case["config"], **(config_over or {})))
    x0 = case["x0"] if x0 is None else x0
    x, f, g, p = solver.minimize(_objective(amd, case), torch.from_numpy(np.ascontiguousarray(x0)).to("cuda:0"),
                                 trace=trace)
    torch.cuda.synchronize()
    return (x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)), solver


def _assert_same_bits(dev, twin, what):
    x, f, g, p = dev
    tx, tf, tg, tp = twin[:4]
    assert x.tobytes() == tx.tobytes(), what + ": x"
    assert f.tobytes() == tf.tobytes(), what + ": f"
    assert g.tobytes() == tg.tobytes(), what + ": g"
    for k in FIELDS:
        assert p[k].tobytes() == tp[k].tobytes(), (what, k, p[k], tp[k])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_matches_twin_in_every_mapping(case):
    n = case["x0"].shape[1]
    for W in (8, 16, 32, 64):
        if W < n:
            continue
        dev, solver = _device_solve(case, lanes=W)
        assert solver.last_launch()["lanes_per_problem"] == W
        twin = T.twin_solve(int(case["objective"]), case["x0"], case["params"], case["stop"], case["config"],
                            order=T.DEVICE_ORDER, W=W)
        _assert_same_bits(dev, twin, "%s W=%d" % (case["name"], W))
    if int(case["config"]["mode"][0]) == T.VALUE:
        assert not dev[2].any() and not dev[3]["gradient_norm"].any()   # g is zeros, gradient_norm stays 0


def test_default_mapping_is_the_padded_width():
    for name, W in (("rosenbrock_n08_solver_value", 8), ("rosenbrock_n09_solver_value", 16),
                    ("rosenbrock_n33_solver_value", 64)):
        _, solver = _device_solve(BY_NAME[name])
        assert solver.last_launch()["lanes_per_problem"] == W


FIRST_CASES = [c for c in CASES if c["name"].endswith("_first")]


@pytest.mark.parametrize("case", FIRST_CASES, ids=[c["name"] for c in FIRST_CASES])
def test_value_and_first_mode_agree(case):
    """With the gradient test off the first-mode solve walks the value-mode one: the same iterates, the same f bit for
    bit (the value-only entry has eval's reduction), at every traced iteration."""
    import torch
    import cppnumericalsolvers_amd as amd
    n = case["x0"].shape[1]
    out = {}
    for mode in (T.VALUE, T.FIRST):
        trace = amd.Trace([0, 3], capacity=512, n=n, device=torch.device("cuda", 0), with_x=True)
        dev, _ = _device_solve(case, trace=trace, stop_over=dict(gradient_norm=0.0), config_over=dict(mode=mode))
        out[mode] = (dev, [trace.history(s) for s in (0, 1)])
    (vx, vf, vg, vp), vh = out[T.VALUE]
    (fx, ff, fg, fp), fh = out[T.FIRST]
    assert vx.tobytes() == fx.tobytes() and vf.tobytes() == ff.tobytes()
    for k in ("status", "num_iterations", "nfev", "x_delta", "f_delta"):
        assert vp[k].tobytes() == fp[k].tobytes(), k
    for (vrec, vxs, _), (frec, fxs, _) in zip(vh, fh):
        assert len(vrec) == len(frec) and len(vrec) > 0
        assert vrec["value"].tobytes() == frec["value"].tobytes()
        assert np.asarray(vxs).tobytes() == np.asarray(fxs).tobytes()
    assert fg.any() and not vg.any()


TRAJECTORY_CASES = [c for c in CASES if "trajectory" in c]


@pytest.mark.parametrize("case", TRAJECTORY_CASES, ids=[c["name"] for c in TRAJECTORY_CASES])
def test_trajectory_matches_reference_callback(case):
    """The per-iteration states the device traces (what the callback replay hands a user) against the states the
    reference's own step callback saw — the bar of tests/test_gpu_trust_region.py: the same number of iterations, the
    same status at every one, value, x_delta, f_delta, gradient_norm and the iterate within 1e-6."""
    import torch
    import cppnumericalsolvers_amd as amd
    n = case["x0"].shape[1]
    trace = amd.Trace([0], capacity=1024, n=n, device=torch.device("cuda", 0), with_x=True)
    _device_solve(case, trace=trace)
    rec, xs, _ = trace.history(0)
    ref, ref_x = case["trajectory"], case["trajectory_x"]
    print(case["name"], "iterations", len(rec), len(ref))
    assert len(rec) == len(ref), (case["name"], len(rec), len(ref))
    assert (rec["num_iterations"] == ref[:, 0]).all()
    assert (rec["status"] == ref[:, 1]).all(), (case["name"], rec["status"], ref[:, 1])
    for col, k in enumerate(("value", "x_delta", "f_delta", "gradient_norm"), start=2):
        print(case["name"], k, float(np.max(np.abs(rec[k] - ref[:, col]))))
        np.testing.assert_allclose(rec[k], ref[:, col], rtol=0, atol=1e-6, err_msg="%s %s" % (case["name"], k))
    np.testing.assert_allclose(xs, ref_x, rtol=0, atol=1e-6, err_msg=case["name"])


def test_python_driver_equals_host_entry():
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    case = BY_NAME["rosenbrock_n09_solver_first"]
    dev, _ = _device_solve(case)
    solver = amd.BatchedNelderMead(stopping_progress=_stop(capi, case["stop"]), **_config(case["config"]))
    hx, hf, hg, hp = solver.minimize_host(amd.Rosenbrock(), case["x0"])
    assert dev[0].tobytes() == hx.tobytes() and dev[1].tobytes() == hf.tobytes() and dev[2].tobytes() == hg.tobytes()
    assert dev[3].tobytes() == hp.tobytes()


def test_verify_scenarios_over_the_drop_in_header():
    """tests/nelder_mead/nm_header_test.cc: RosenbrockValue from (15, 8) and (-1, 2) through
    include/cppoptlib/solver/nelder_mead.h on the device, the reference's own bar |f(x*)| < 1e-4 (built by build())."""
    exe = os.path.join(T.NM_DIR, "_build", "nm_header_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def _library(name):
    return os.path.join(T.REPO, "cppnumericalsolvers_amd", name)


@pytest.mark.parametrize("n", [2, 3])
def test_l1_example_library(n):
    """f(x) = sum |x_i - c_i| + 0.5 sum (x_i - c_i)^2 as a value-only user functor (examples/user_objective_l1,
    libmi355_lbfgs_nm.so): the minimiser c, where f is not differentiable, within 1e-3 in the inf-norm, not by the
    iteration limit; bit for bit the device-order twin.

    The setting is the one in which the simplex method is known to converge: the standard coefficients (1, 2, 0.5, 0.5),
    a strictly convex function in low dimension (n = 2, 3), and a stopping rule that does not count the steps on which
    the returned best vertex stands still while the simplex contracts around it (plateau test off, 50 x_delta strikes).
    The reference's own coefficients (xi = 20, gamma = 0.1) with its default stop end 0.2 - 2 away from c on this
    function, in the reference-exact twin as on the device: that is the algorithm, not the kernel."""
    import cppnumericalsolvers_amd as amd
    rng = np.random.default_rng(20261017 + n)
    B = 8
    c = rng.uniform(-1.0, 1.0, n)
    x0 = rng.uniform(-2.0, 2.0, (B, n))
    case = dict(objective=np.int32(T.L1_QUADRATIC), x0=x0, params=c,
                stop=T.make_stop(**{**T.STOP_PRESETS["solver"], "x_delta_violations": 50, "past": 0}),
                config=T.make_config(xi=2.0, gamma=0.5))
    ctx = amd.Context(0, library=_library("libmi355_lbfgs_nm.so"))
    dev, _ = _device_solve(case, context=ctx)
    x, f, g, p = dev
    print("l1 n=%d: max |x - c| =" % n, float(np.max(np.abs(x - c))), "status", p["status"], "iterations",
          p["num_iterations"])
    assert (p["status"] != 1).all()
    assert np.max(np.abs(x - c)) <= 1e-3
    _assert_same_bits(dev, T.twin_solve(T.L1_QUADRATIC, x0, c, case["stop"], case["config"], order=T.DEVICE_ORDER, W=8),
                      "l1 quadratic")
    # a value-only functor has no first mode
    from cppnumericalsolvers_amd import capi
    with pytest.raises(capi.EngineError) as e:
        _device_solve(case, context=ctx, config_over=dict(mode=T.FIRST))
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    assert b"value-only" in ctx._lib.mi355_lbfgs_last_error()


def test_refusals_are_clean_errors():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi

    def refused(match, solver, objective, x0, **kw):
        with pytest.raises(capi.EngineError, match=match) as e:
            solver.minimize(objective, x0, **kw)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT

    x65 = torch.zeros((2, 65), dtype=torch.float64, device="cuda:0")
    refused("n <= 64", amd.BatchedNelderMead(), amd.Rosenbrock(), x65)
    x12 = torch.zeros((2, 12), dtype=torch.float64, device="cuda:0")
    refused("cover n", amd.BatchedNelderMead(lanes_per_problem=8), amd.Rosenbrock(), x12)
    refused("8, 16, 32 or 64", amd.BatchedNelderMead(lanes_per_problem=24), amd.Rosenbrock(), x12)
    x4 = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    solver = amd.BatchedNelderMead()
    solver.arithmetic = capi.ARITH_FMA
    refused("exact arithmetic", solver, amd.Rosenbrock(), x4)
    A, y = np.ones((3, 4)), np.zeros((2, 3))
    refused("Rosenbrock, DiagQuadratic", amd.BatchedNelderMead(), amd.SquaredErrorRidge(A, 0.1), x4,
            per_problem=torch.from_numpy(y).to("cuda:0"))
    with pytest.raises(ValueError):
        amd.BatchedNelderMead(mode="second")
    # a library built without Nelder-Mead kernels for its user objective
    ctx = amd.Context(0, library=_library("libmi355_lbfgs_svm.so"))
    with pytest.raises(capi.EngineError) as e:
        amd.BatchedNelderMead(context=ctx).minimize(amd.Objective(100, np.zeros(1), "svm"), x4)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    assert b"no Nelder-Mead kernel" in ctx._lib.mi355_lbfgs_last_error()


def test_batch_larger_than_a_capped_grid(monkeypatch):
    """64 problems at n = 7 with the resident grid capped to one workgroup (eight segments): every segment goes back to
    the work queue eight times; equal to the uncapped run bit for bit, and to the twin."""
    import cppnumericalsolvers_amd as amd
    rng = np.random.default_rng(20261017)
    x0 = rng.uniform(-2.0, 2.0, (64, 7))
    case = dict(BY_NAME["rosenbrock_n07_solver_first"], x0=x0)
    free, free_solver = _device_solve(case)
    assert free_solver.last_launch()["blocks"] == 8
    monkeypatch.setenv(CAP_ENV, "1")
    ctx = amd.Context(0)
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        capped, solver = _device_solve(case, context=ctx)
        assert solver.last_launch()["blocks"] == 1
    finally:
        ctx.close()
    for a, b in zip(free, capped):
        assert a.tobytes() == b.tobytes()
    _assert_same_bits(capped, T.twin_solve(T.ROSENBROCK, x0, None, case["stop"], case["config"], order=T.DEVICE_ORDER, W=8),
                      "capped grid")
