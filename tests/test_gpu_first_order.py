"""GradientDescent and ConjugatedGradientDescent on the MI355X (csrc/first_order_kernel.hpp): bit for bit the CPU twin in
device order on every recorded case and under several lane mappings, within 1e-6 of the reference's recorded solves with
the same status on the unmarked cases, the traced trajectory against the reference's callback states, the Python drivers
equal to the host entry points, the quartic user functor, the drop-in headers, clean refusals, and the work queue under a
capped grid."""
import os
import subprocess

import numpy as np
import pytest

import fo_cases
import fo_lib as T
import tr_queue as Q

pytestmark = pytest.mark.gpu
CASES = fo_cases.load_cases()
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"


def _objective(amd, case):
    obj = int(case["objective"])
    if obj == T.ROSENBROCK:
        return amd.Rosenbrock()
    if obj == T.DIAG_QUADRATIC:
        n = case["x0"].shape[1]
        return amd.DiagQuadratic(case["params"][:n], float(case["params"][n]))
    return amd.Objective(100, np.zeros(0), "quartic")


def _stop(capi, rec):
    s = capi.Stop()
    for k in T.STOP_DTYPE.names:
        setattr(s, k, rec[k][0].item())
    return s


def _library(name):
    return os.path.join(T.REPO, "cppnumericalsolvers_amd", name)


_quartic_ctx = []


def _context(case):
    """The default library's shared context, or — the quartic is a user functor — one on libmi355_lbfgs_tr.so."""
    import cppnumericalsolvers_amd as amd
    if int(case["objective"]) != T.QUARTIC:
        return None
    if not _quartic_ctx:
        _quartic_ctx.append(amd.Context(0, library=_library("libmi355_lbfgs_tr.so")))
    return _quartic_ctx[0]


def _solver(method, stop, context=None, lanes=0, elems=0, config=None):
    import cppnumericalsolvers_amd as amd
    if method == T.GRADIENT_DESCENT:
        return amd.BatchedGradientDescent(stopping_progress=stop, lanes_per_problem=lanes, elems_per_lane=elems,
                                          context=context)
    kw = {} if config is None else {"armijo_" + k: config[k][0].item() for k in T.CONFIG_FIELDS}
    return amd.BatchedConjugatedGradientDescent(stopping_progress=stop, lanes_per_problem=lanes, elems_per_lane=elems,
                                                context=context, **kw)


def _device_solve(case, lanes=0, elems=0, trace=None):
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    solver = _solver(int(case["method"]), _stop(capi, case["stop"]), _context(case), lanes, elems, case["config"])
    x, f, g, p = solver.minimize(_objective(amd, case), torch.from_numpy(case["x0"]).to("cuda:0"), trace=trace)
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


def _twin(case, order=T.DEVICE_ORDER, width=None):
    return T.twin_solve(int(case["method"]), int(case["objective"]), case["x0"], case["params"], case["stop"],
                        case["config"], order=order, width=width)


def _assert_same_bits(a, b, what):
    diff = Q.same_bits(a, b)
    assert diff is None, "%s: %s" % (what, diff)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_matches_twin_and_reference(case):
    """(The quartic cases run through the user-objective library.)"""
    out = _device_solve(case)
    _assert_same_bits(out, _twin(case), case["name"])
    x, f, g, p = out
    rp = case["progress"]
    if int(case["marked"]):
        # the two summation orders end this case's solves at different iterates (fo_cases.py): f* where both converged
        both = np.isin(p["status"], fo_cases.CONVERGED) & np.isin(rp["status"], fo_cases.CONVERGED)
        np.testing.assert_allclose(f[both], case["f"][both], rtol=0, atol=1e-6, err_msg=case["name"])
        return
    assert (p["status"] == rp["status"]).all(), (case["name"], p["status"], rp["status"])
    # (an overflowing start stays at a non-finite f in both: equal infinities / NaNs compare equal here)
    np.testing.assert_allclose(f, case["f"], rtol=0, atol=1e-6, err_msg=case["name"])
    ref_x = fo_cases.reference_x(case, _twin(case, order=T.REF_ORDER)[0])
    np.testing.assert_allclose(x, ref_x, rtol=0, atol=1e-6, err_msg=case["name"])


@pytest.mark.parametrize("name,mappings", [
    ("gd_rosenbrock_n007_default", [(8, 1), (64, 1), (0, 0)]), ("cg_rosenbrock_n007_default", [(8, 1), (64, 1), (0, 0)]),
    ("gd_rosenbrock_n032_parity", [(32, 1), (64, 1), (0, 0)]), ("cg_rosenbrock_n032_parity", [(32, 1), (64, 1), (0, 0)]),
    ("gd_diag_quadratic_n100", [(64, 2), (64, 4), (0, 0)]), ("cg_diag_quadratic_n100", [(64, 2), (64, 4), (0, 0)])])
def test_lane_mappings_same_bits(name, mappings):
    """Padding coordinates add zeros to every tree: the padded width, a wider mapping and the library's own choice
    (lanes_per_problem = 0) give the same bytes."""
    case = next(c for c in CASES if c["name"] == name)
    first = _device_solve(case, *mappings[0])
    for lanes, elems in mappings[1:]:
        _assert_same_bits(first, _device_solve(case, lanes, elems), "%s %dx%d" % (name, lanes, elems))


TRAJECTORY_CASES = [c for c in CASES if "trajectory" in c]


@pytest.mark.parametrize("case", TRAJECTORY_CASES, ids=[c["name"] for c in TRAJECTORY_CASES])
def test_trajectory_matches_reference_callback(case):
    """The per-iteration states the device traces (what the callback replay hands a user) against the states the
    reference's own step callback saw: the same number of iterations, the same status at every one, value, x_delta,
    f_delta, gradient_norm and the iterate within 1e-6."""
    import torch
    import cppnumericalsolvers_amd as amd
    n = case["x0"].shape[1]
    trace = amd.Trace([0], capacity=1024, n=n, device=torch.device("cuda", 0), with_x=True)
    _device_solve(case, trace=trace)
    rec, xs, _ = trace.history(0)
    ref, ref_x = case["trajectory"], case["trajectory_x"]
    assert len(rec) == len(ref), (case["name"], len(rec), len(ref))
    assert (rec["num_iterations"] == ref[:, 0]).all()
    assert (rec["status"] == ref[:, 1]).all(), (case["name"], rec["status"], ref[:, 1])
    for col, k in enumerate(("value", "x_delta", "f_delta", "gradient_norm"), start=2):
        np.testing.assert_allclose(rec[k], ref[:, col], rtol=0, atol=1e-6, err_msg="%s %s" % (case["name"], k))
    np.testing.assert_allclose(xs, ref_x, rtol=0, atol=1e-6, err_msg=case["name"])


@pytest.mark.parametrize("name", ["gd_rosenbrock_n032_default", "cg_rosenbrock_n032_default"])
def test_python_driver_equals_host_entry(name):
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    case = next(c for c in CASES if c["name"] == name)
    solver = _solver(int(case["method"]), _stop(capi, case["stop"]), config=case["config"])
    _assert_same_bits(_device_solve(case), solver.minimize_host(amd.Rosenbrock(), case["x0"]), "minimize_host")
    ll = solver.last_launch()
    assert ll["lanes_per_problem"] == 32 and ll["elems_per_lane"] == 1, ll


@pytest.mark.parametrize("method", [T.GRADIENT_DESCENT, T.CONJUGATED_GRADIENT_DESCENT], ids=["gd", "cg"])
def test_refusals_are_clean_errors(method):
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    x257 = torch.zeros((2, 257), dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.EngineError, match="n <= 256") as e:
        _solver(method, None).minimize(amd.Rosenbrock(), x257)
    assert e.value.code == capi.ERR_UNSUPPORTED
    x4 = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    solver = _solver(method, None)
    solver.arithmetic = capi.ARITH_FMA
    with pytest.raises(capi.EngineError, match="exact arithmetic") as e:
        solver.minimize(amd.Rosenbrock(), x4)
    assert e.value.code == capi.ERR_UNSUPPORTED
    A = np.ones((3, 4))
    y = np.zeros((2, 3))
    with pytest.raises(capi.EngineError, match="without LDS data") as e:
        _solver(method, None).minimize(amd.SquaredErrorRidge(A, 0.1), x4, per_problem=torch.from_numpy(y).to("cuda:0"))
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.EngineError, match="cover n") as e:
        _solver(method, None, lanes=8).minimize(amd.Rosenbrock(), torch.zeros((2, 9), dtype=torch.float64,
                                                                              device="cuda:0"))
    assert e.value.code == capi.ERR_INVALID_ARGUMENT


def test_library_without_first_order_kernels_refuses():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    ctx = amd.Context(0, library=_library("libmi355_lbfgs_svm.so"))   # user objective 100 built for Lbfgs only
    x0 = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    for method in (T.GRADIENT_DESCENT, T.CONJUGATED_GRADIENT_DESCENT):
        with pytest.raises(capi.EngineError) as e:
            _solver(method, None, context=ctx).minimize(amd.Objective(100, np.zeros(1), "svm"), x0)
        assert e.value.code == capi.ERR_UNSUPPORTED
        # (capi.check reads the text from the first loaded library that holds one: ask the failing library itself)
        assert b"no first-order kernel" in ctx._lib.mi355_lbfgs_last_error()
    ctx.close()


def test_reference_scenarios_over_the_drop_in_headers():
    """tests/first_order/fo_header_test.cc: the four verify.cc scenarios with the reference's
    EXPECT_NEAR(0, f(x*), 1e-4), a callback count and the batched entry, through the two drop-in headers (built by
    build())."""
    exe = os.path.join(T.FO_DIR, "_build", "fo_header_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("method", [T.GRADIENT_DESCENT, T.CONJUGATED_GRADIENT_DESCENT], ids=["gd", "cg"])
def test_work_queue_refetch_under_a_capped_grid(method, monkeypatch, gpu_solver_factory):
    """600 mixed Rosenbrock-8 rows (converging starts, far starts, rows of exact ones, rows of 1e100) through a grid capped
    at 2 workgroups: 16 resident segments, each fetching some 37 problems of very different length in a row, under a
    stop capped at 40 iterations so that the batch runs in seconds.  The twin solves every row on its own: a queue or
    reset bug is a bit difference.  (gpu_solver_factory is asked for first, so that the session's shared context is
    never created under the cap.)"""
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    n, B, cap = 8, 600, 2
    x0 = Q.mixed_rosenbrock_batch(n, B, 20261019)[0]
    stop = capi.default_stop()
    stop.num_iterations = 40
    monkeypatch.setenv(CAP_ENV, str(cap))
    ctx = amd.Context(0)
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        import torch
        solver = _solver(method, stop, context=ctx)
        x, f, g, p = solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to("cuda:0"))
        torch.cuda.synchronize()
        out = (x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p))
        ll = solver.last_launch()
        assert ll["blocks"] == cap and ll["lanes_per_problem"] == 8, ll
        assert B >= 4 * cap * (64 // 8)
    finally:
        ctx.close()
    twin = T.twin_solve_threaded(method, T.ROSENBROCK, x0, None,
                                 T.make_stop(**{**T.STOP_PRESETS["default"], "num_iterations": 40}),
                                 order=T.DEVICE_ORDER, width=8)
    _assert_same_bits(out, twin, "capped grid")
    assert len(set(out[3]["num_iterations"].tolist())) > 3       # solves of different lengths are in the batch
