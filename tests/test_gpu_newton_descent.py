"""NewtonDescent on the MI355X (csrc/newton_descent_kernel.hpp): bit for bit the CPU twin in device order on every
recorded case and under two lane mappings, within 1e-6 of the reference's recorded solves with the same status on the
unmarked cases, the traced trajectory against the reference's callback states, the Python driver equal to the host entry
point, the quartic user functor, the dense-Hessian user functor (the LU with far pivots, ties and fill-in, asymmetric
Hessians, the condition test at n up to 64, an all-zero pivot column), the drop-in header, clean refusals, and the work
queue under a capped grid."""
import os
import subprocess

import numpy as np
import pytest

import dense_cases as D
import nd_cases
import nd_lib as T
import tr_queue as Q

pytestmark = pytest.mark.gpu
CASES = nd_cases.load_cases()
FIELDS = ("status", "num_iterations", "nfev", "sum_k", "x_delta", "f_delta", "gradient_norm")
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"


def _objective(amd, case):
    obj = int(case["objective"])
    if obj == T.ROSENBROCK:
        return amd.Rosenbrock()
    if obj == T.DIAG_QUADRATIC:
        n = case["x0"].shape[1]
        return amd.DiagQuadratic(case["params"][:n], float(case["params"][n]))
    if obj == T.DENSE:
        return amd.Objective(101, case["params"], "dense_quartic")
    return amd.Objective(100, np.zeros(0), "quartic")


def _stop(capi, rec):
    s = capi.Stop()
    for k in T.STOP_DTYPE.names:
        setattr(s, k, rec[k][0].item())
    return s


def _config(rec):
    return {k: rec[k][0].item() for k in T.CONFIG_FIELDS}


def _library(name):
    return os.path.join(T.REPO, "cppnumericalsolvers_amd", name)


_quartic_ctx = []


def _context(case):
    """The default library's shared context, or — the quartic and the dense quartic are user functors — one on
    libmi355_lbfgs_tr.so."""
    import cppnumericalsolvers_amd as amd
    if int(case["objective"]) not in (T.QUARTIC, T.DENSE):
        return None
    if not _quartic_ctx:
        _quartic_ctx.append(amd.Context(0, library=_library("libmi355_lbfgs_tr.so")))
    return _quartic_ctx[0]


def _device_solve(case, lanes=0, trace=None):
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    solver = amd.BatchedNewtonDescent(stopping_progress=_stop(capi, case["stop"]), lanes_per_problem=lanes,
                                      condition_hessian=float(case["condition_stop"]), context=_context(case),
                                      **_config(case["config"]))
    x, f, g, p = solver.minimize(_objective(amd, case), torch.from_numpy(case["x0"]).to("cuda:0"), trace=trace)
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


def _twin(case, W=None):
    return T.twin_solve(int(case["objective"]), case["x0"], case["params"], case["stop"], case["config"],
                        float(case["condition_stop"]), order=T.DEVICE_ORDER, W=W)


def _assert_same_bits(a, b, what):
    diff = Q.same_bits(a, b)
    assert diff is None, "%s: %s" % (what, diff)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_matches_twin_and_reference(case):
    """(The quartic and the dense cases run through the user-objective library.  A dense case above n = 33 keeps a digest
    of the reference's x*: the twin in reference order, checked against the digest, stands in for it.)"""
    out = _device_solve(case)
    _assert_same_bits(out, _twin(case), case["name"])
    x, f, g, p = out
    rp = case["progress"]
    if "x" not in case:
        case = {**case, "x": D.reference_x(case, T.twin_solve(int(case["objective"]), case["x0"], case["params"],
                                                              case["stop"], case["config"],
                                                              float(case["condition_stop"]))[0])}
    if int(case["marked"]):
        # the two summation orders end this case's solves at different iterates (nd_cases.py): f* where both converged
        both = np.isin(p["status"], nd_cases.CONVERGED) & np.isin(rp["status"], nd_cases.CONVERGED)
        np.testing.assert_allclose(f[both], case["f"][both], rtol=0, atol=1e-6, err_msg=case["name"])
        return
    assert (p["status"] == rp["status"]).all(), (case["name"], p["status"], rp["status"])
    # (an overflowing start stays at f = inf in both: equal infinities compare equal here)
    np.testing.assert_allclose(f, case["f"], rtol=0, atol=1e-6, err_msg=case["name"])
    np.testing.assert_allclose(x, case["x"], rtol=0, atol=1e-6, err_msg=case["name"])


@pytest.mark.parametrize("name", ["rosenbrock_n07_default", "rosenbrock_n32_parity", "edge_condition_hessian",
                                  "dense_spd_n09_default", "dense_spd_n33_default"])
def test_lane_mappings_same_bits(name):
    """Padding lanes add zeros to every butterfly: 64 lanes per problem give the bytes of the padded width, and the
    library's own choice (lanes_per_problem = 0) gives them too."""
    case = next(c for c in CASES if c["name"] == name)
    padded = _device_solve(case, lanes=T.padded_width(case["x0"].shape[1]))
    _assert_same_bits(padded, _device_solve(case, lanes=64), name)
    _assert_same_bits(padded, _device_solve(case), name + " (library's choice)")


def _nan_blind(a):
    """(x, f, g, progress) with every NaN replaced by one bit pattern: an invalid operation yields the default NaN of the
    machine it runs on, and the sign bit of that differs between the host and the device"""
    def fix(v):
        v = np.array(v, dtype=np.float64)
        v[np.isnan(v)] = np.nan
        return v
    p = a[3].copy()
    for k in ("x_delta", "f_delta", "gradient_norm"):
        p[k] = fix(p[k])
    return fix(a[0]), fix(a[1]), fix(a[2]), p


def test_zero_pivot_column_matches_twin():
    """S e_0 = 0, kappa = 0, safe_guard = 0: column 0 of the LU has no non-zero entry (the `best == 0` branch: no
    interchange, no division) and the solve divides by lu(0, 0) = 0, so the iterates are infinite or NaN from the first
    step.  The reference's safe_guard is a constant 1e-5: this is the device against its twin only, three iterations,
    every field bit for bit except that a NaN equals a NaN."""
    case = D.zero_column_case()
    out = _device_solve(case)
    assert not np.isfinite(out[0]).all()
    _assert_same_bits(_nan_blind(out), _nan_blind(_twin(case)), case["name"])


@pytest.mark.parametrize("n", sorted(D.CHAIN_CASES))
def test_strongly_asymmetric_hessian_matches_twin(n):
    """dense_cases.chain_case: an antisymmetric part of 2^60 and more in S, so that the chain of the search,
    v_j = sum_i (k d_i) H(i, j), gives another step length if it walks row j for column j (the twin with that bug planted
    changes its bytes on this case: tests/test_newton_descent_twin.py).  The device against its twin, three iterations,
    every field bit for bit."""
    case = D.chain_case(n)
    _assert_same_bits(_device_solve(case), _twin(case), case["name"])


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


def test_python_driver_equals_host_entry():
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    case = next(c for c in CASES if c["name"] == "rosenbrock_n32_default")
    solver = amd.BatchedNewtonDescent(stopping_progress=_stop(capi, case["stop"]), **_config(case["config"]))
    hx, hf, hg, hp = solver.minimize_host(amd.Rosenbrock(), case["x0"])
    _assert_same_bits(_device_solve(case), (hx, hf, hg, hp), "minimize_host")


def test_refusals_are_clean_errors():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    x65 = torch.zeros((2, 65), dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.EngineError, match="n <= 64") as e:
        amd.BatchedNewtonDescent().minimize(amd.Rosenbrock(), x65)
    assert e.value.code == capi.ERR_UNSUPPORTED
    x4 = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    solver = amd.BatchedNewtonDescent()
    solver.arithmetic = capi.ARITH_FMA
    with pytest.raises(capi.EngineError, match="exact arithmetic") as e:
        solver.minimize(amd.Rosenbrock(), x4)
    assert e.value.code == capi.ERR_UNSUPPORTED
    A = np.ones((3, 4))
    y = np.zeros((2, 3))
    with pytest.raises(capi.EngineError, match="device Hessian") as e:
        amd.BatchedNewtonDescent().minimize(amd.SquaredErrorRidge(A, 0.1), x4,
                                            per_problem=torch.from_numpy(y).to("cuda:0"))
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_library_without_newton_descent_kernels_refuses():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    ctx = amd.Context(0, library=_library("libmi355_lbfgs_svm.so"))   # user objective 100 built for Lbfgs only
    x0 = torch.zeros((2, 4), dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.EngineError) as e:
        amd.BatchedNewtonDescent(context=ctx).minimize(amd.Objective(100, np.zeros(1), "svm"), x0)
    assert e.value.code == capi.ERR_UNSUPPORTED
    # (capi.check reads the text from the first loaded library that holds one: ask the failing library itself)
    assert b"no Newton-descent kernel" in ctx._lib.mi355_lbfgs_last_error()
    ctx.close()


def test_reference_scenarios_over_the_drop_in_header():
    """tests/newton_descent/nd_header_test.cc: the two verify.cc scenarios with the reference's
    EXPECT_NEAR(0, f(x*), 1e-4), a callback count and the batched entry, through
    include/cppoptlib/solver/newton_descent.h (built by build())."""
    exe = os.path.join(T.ND_DIR, "_build", "nd_header_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_work_queue_refetch_under_a_capped_grid(monkeypatch, gpu_solver_factory):
    """600 mixed Rosenbrock-8 rows (converging starts, stalled searches of hundreds of trials at s = 2 and 3, rows of exact
    ones, rows of 1e100) through a grid capped at 2 workgroups: 16 resident segments, each fetching some 37 problems of
    very different length in a row.  The twin solves every row on its own: a queue or reset bug is a bit difference.
    (gpu_solver_factory is asked for first, so that the session's shared context is never created under the cap.)"""
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    n, B, cap = 8, 600, 2
    x0 = Q.mixed_rosenbrock_batch(n, B, 20261018)[0]
    monkeypatch.setenv(CAP_ENV, str(cap))
    ctx = amd.Context(0)
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        import torch
        solver = amd.BatchedNewtonDescent(stopping_progress=capi.default_stop(), context=ctx)
        x, f, g, p = solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to("cuda:0"))
        torch.cuda.synchronize()
        out = (x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p))
        ll = solver.last_launch()
        assert ll["blocks"] == cap and ll["lanes_per_problem"] == 8, ll
        assert B >= 4 * cap * (64 // 8)
    finally:
        ctx.close()
    twin = T.twin_solve_threaded(T.ROSENBROCK, x0, None, T.make_stop(**T.STOP_PRESETS["default"]), order=T.DEVICE_ORDER,
                                 W=8)
    _assert_same_bits(out, twin, "capped grid")
    assert (out[3]["sum_k"] >= 100).any() and (out[3]["status"] == 2).any()      # the stalled searches are in the batch


def test_dense_work_queue_refetch_under_a_capped_grid(monkeypatch, gpu_solver_factory):
    """300 rows of the dense SPD functor at n = 9 through a grid capped at 2 workgroups with 16 lanes per problem: 8
    resident segments, each fetching some 37 problems in a row and factorising every one in the same two LDS matrices.
    Starts of mixed scale (q / 128 with |q| <= 256, and up to 4096 for every third row) give solves of different length.
    The twin solves every row on its own: a matrix, pivot or queue state left over from the previous problem is a bit
    difference.  (gpu_solver_factory is asked for first, so that the session's shared context is never created under the
    cap.)"""
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    n, B, cap = 9, 300, 2
    case = next(c for c in CASES if c["name"] == "dense_spd_n09_default")
    rng = np.random.default_rng(20261018)
    q = rng.integers(-256, 257, (B, n))
    q[::3] = rng.integers(-4096, 4097, (len(q[::3]), n))
    x0 = q.astype(np.float64) / 128.0
    monkeypatch.setenv(CAP_ENV, str(cap))
    ctx = amd.Context(0, library=_library("libmi355_lbfgs_tr.so"))
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        solver = amd.BatchedNewtonDescent(stopping_progress=capi.default_stop(), lanes_per_problem=16, context=ctx)
        x, f, g, p = solver.minimize(_objective(amd, case), torch.from_numpy(x0).to("cuda:0"))
        torch.cuda.synchronize()
        out = (x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p))
        ll = solver.last_launch()
        assert ll["blocks"] == cap and ll["lanes_per_problem"] == 16, ll
        assert B >= 4 * cap * (64 // 16)
    finally:
        ctx.close()
    twin = T.twin_solve_threaded(T.DENSE, x0, case["params"], T.make_stop(**T.STOP_PRESETS["default"]),
                                 order=T.DEVICE_ORDER, W=16)
    _assert_same_bits(out, twin, "capped grid, dense")
    assert len(set(out[3]["num_iterations"].tolist())) > 3
