"""The native fp32 L-BFGS path on the device (mi355_lbfgs_minimize_batch_f32, _host, mi355_lbfgs_eval_batch_f32,
BatchedLbfgs(dtype=torch.float32)) against its CPU twin in device order (tests/lbfgs_f32/f32_twin.hpp), bit for bit, and
against the recorded reference (tests/golden/lbfgs_f32_reference.npz)."""
import ctypes as C

import numpy as np
import pytest

import l32_cases as Cs
import l32_lib as L

pytestmark = pytest.mark.gpu
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
B_SOLVE = 131
_CASES = Cs.all_cases()
_GROUPS = sorted({(c["objective"], c["n"], c["m"]) for c in _CASES})


def _amd():
    import cppnumericalsolvers_amd as amd
    return amd


def _objective(case_or_id, params=None):
    amd = _amd()
    if isinstance(case_or_id, dict):
        params, case_or_id = case_or_id["params"], case_or_id["objective"]
    return amd.Rosenbrock() if case_or_id == L.ROSENBROCK else amd.DiagQuadratic(params[:-1], params[-1])


def _stop(record):
    from cppnumericalsolvers_amd import capi
    s = capi.Stop()
    for name in L.STOP_DTYPE.names:
        setattr(s, name, record[name][0].item())
    return s


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def contexts():
    """the default context and one created under MI355_DEBUG_SOLVE_BLOCKS=1 (every segment fetches again and again)"""
    import os
    amd = _amd()
    assert CAP_ENV not in os.environ
    default = amd.Context(0)
    os.environ[CAP_ENV] = "1"
    try:
        capped = amd.Context(0)
    finally:
        del os.environ[CAP_ENV]
    yield default, capped
    default.close()
    capped.close()


def _solver(ctx, m, stop, **kw):
    import torch
    return _amd().BatchedLbfgs(m=m, stopping_progress=stop, context=ctx, arithmetic="exact", dtype=torch.float32, **kw)


def _device_solve(solver, objective, x0):
    import torch
    x, f, g, p = solver.minimize(objective, _dev(x0))
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), _amd().progress_to_numpy(p)


def _same(got, want, what):
    for name, a, b in zip(("x", "f", "g"), got[:3], want[:3]):
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), "%s: %s differs from the twin" % (what, name)
    for fld in L.PROGRESS_FIELDS:
        assert got[3][fld].tobytes() == want[3][fld].tobytes(), "%s: progress.%s differs from the twin" % (what, fld)


def _tiled(case):
    """the case's starts cycled to B_SOLVE rows, and the twin's results (device order) tiled the same way"""
    R = case["x0"].shape[0]
    idx = np.arange(B_SOLVE) % R
    twin = L.twin_solve(case["objective"], case["m"], case["x0"], case["params"], case["stop"], order=L.DEVICE_ORDER,
                        width=L.padded_width(case["n"]))
    return case["x0"][idx], tuple(a[idx] for a in twin)


# ---- 1. one evaluation per row ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8, 13, 64, 65, 130, 256])
@pytest.mark.parametrize("objective", [L.ROSENBROCK, L.DIAG_QUADRATIC])
def test_eval_is_the_twin(contexts, objective, n):
    import torch
    x = Cs._x0_host(64, n, "wide", 77 + n).astype(np.float32)
    params = Cs._coefficients(n, 5 + n) if objective == L.DIAG_QUADRATIC else None
    solver = _solver(contexts[0], 6, None)
    f, g = solver.evaluate(_objective(objective, params), _dev(x))
    torch.cuda.synchronize()
    tf, tg = L.twin_eval(objective, x, params, width=L.padded_width(n))
    assert f.dtype == torch.float32 and f.cpu().numpy().tobytes() == tf.tobytes()
    assert g.cpu().numpy().tobytes() == tg.tobytes()


# ---- 2. the solve, every case of the CPU suite -------------------------------------------------------------------------
@pytest.mark.parametrize("objective,n,m", _GROUPS)
def test_solve_is_the_twin(contexts, objective, n, m):
    """Device entry and host entry on the default grid, device entry under a one-workgroup grid (B = 131: every segment
    fetches 131 / (64 / W) times, so the in-place reset of the ring, gamma, the counters and the plateau ring runs)."""
    default, capped = contexts
    for case in _CASES:
        if (case["objective"], case["n"], case["m"]) != (objective, n, m):
            continue
        x0, twin = _tiled(case)
        obj, stop = _objective(case), _stop(case["stop"])
        s = _solver(default, m, stop)
        _same(_device_solve(s, obj, x0), twin, case["name"] + " (device entry)")
        _same(s.minimize_host(obj, x0), twin, case["name"] + " (host entry)")
        c = _solver(capped, m, stop)
        got = _device_solve(c, obj, x0)
        assert c.last_launch()["blocks"] == 1
        _same(got, twin, case["name"] + " (one workgroup)")


def test_host_entry_in_chunks(contexts, monkeypatch):
    """the host entry through several staging chunks (MI355_HOST_STAGE_BYTES at its floor of 64 KiB)"""
    case = next(c for c in _CASES if c["name"] == "diag_quadratic_n65_m6_default")
    R = case["x0"].shape[0]
    idx = np.arange(700) % R
    twin = L.twin_solve(case["objective"], case["m"], case["x0"], case["params"], case["stop"], order=L.DEVICE_ORDER)
    monkeypatch.setenv("MI355_HOST_STAGE_BYTES", str(64 << 10))
    s = _solver(contexts[0], case["m"], _stop(case["stop"]))
    _same(s.minimize_host(_objective(case), case["x0"][idx]), tuple(a[idx] for a in twin), "chunked host entry")


# ---- 3. mapping independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mappings", [(13, [(16, 1), (32, 1), (64, 1)]), (100, [(64, 2), (64, 4)])])
def test_mapping_independence(contexts, n, mappings):
    x0 = Cs._starts(n, 4242)
    results = []
    for W, E in mappings:
        s = _solver(contexts[0], 6, None, lanes_per_problem=W, elems_per_lane=E)
        results.append(_device_solve(s, _objective(L.ROSENBROCK), x0))
        ll = s.last_launch()
        assert (ll["lanes_per_problem"], ll["elems_per_lane"]) == (W, E)
    for r in results[1:]:
        _same(r, results[0], "mapping")
    # ... and the widest is its twin at that width
    W, E = mappings[-1]
    _same(results[-1], L.twin_solve(L.ROSENBROCK, 6, x0, order=L.DEVICE_ORDER, width=W * E), "widest mapping")


# ---- 4. permutation ------------------------------------------------------------------------------------------------------
def test_permuted_batch_gives_permuted_results(contexts):
    n = 33
    x0 = np.concatenate([Cs._x0_host(100, n, "std", 9), Cs._x0_host(97, n, "wide", 10)]).astype(np.float32)
    perm = np.random.default_rng(3).permutation(len(x0))
    s = _solver(contexts[0], 6, None)
    a = _device_solve(s, _objective(L.ROSENBROCK), x0)
    b = _device_solve(s, _objective(L.ROSENBROCK), x0[perm])
    _same(b, tuple(t[perm] for t in a), "permutation")
    c = _solver(contexts[1], 6, None)
    _same(_device_solve(c, _objective(L.ROSENBROCK), x0[perm]), b, "permutation under one workgroup")


# ---- 5. the recorded reference ---------------------------------------------------------------------------------------------
def test_against_the_recorded_reference(contexts):
    """The reference's criterion f < 1e-4 from verify.cc's two starts, and on every DiagQuadratic case and those two
    starts |x - x_ref|_inf and |f - f_ref| within twice the gap between the twin's two summation orders as
    tests/test_lbfgs_f32_twin.py::test_gap_between_the_two_orders measured it on the recorded draw:
    max |dx|_inf = 3.3945e-4, max |df| = 1.0681e-4 (l32_cases.ORDER_GAP_X / ORDER_GAP_F).  The factor two allows a re-record
    on another draw; on one draw the device's distance is the twin's (test_solve_is_the_twin)."""
    recorded = Cs.load_recorded(_CASES)
    worst_x = worst_f = 0.0
    compared = 0
    for case in _CASES:
        if not Cs.compared_as_numbers(case):
            continue
        s = _solver(contexts[0], case["m"], _stop(case["stop"]))
        x, f, _, _ = _device_solve(s, _objective(case), case["x0"])
        ref = recorded[case["name"]]
        if case["name"] == "verify_2d":
            assert np.all(np.abs(f) < Cs.VERIFY_BOUND), f
        worst_x = max(worst_x, float(np.abs(x.astype(np.float64) - ref["x"]).max()))
        worst_f = max(worst_f, float(np.abs(f.astype(np.float64) - ref["f"]).max()))
        compared += 1
    print("device against the recorded reference: max |dx|_inf = %.4e, max |df| = %.4e over %d cases"
          % (worst_x, worst_f, compared))
    assert compared == len(Cs.DIMS) * len(Cs.HISTORIES) * len(Cs.STOPS) + 1
    assert worst_x <= 2 * Cs.ORDER_GAP_X and worst_f <= 2 * Cs.ORDER_GAP_F


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
UNSUPPORTED, INVALID = -4, -1
_PREFIX = "Lbfgs float32"
REFUSALS = [
    ("objective", dict(objective=2), UNSUPPORTED,
     " is built for the Rosenbrock and DiagQuadratic objectives (no user functors, ridge forms or composites)"),
    ("linesearch", dict(linesearch=1), UNSUPPORTED, " is built with the More-Thuente line search only"),
    ("arithmetic", dict(arithmetic=2), UNSUPPORTED, " is built for the exact arithmetic only (no MI355_ARITH_FMA)"),
    ("history_placement", dict(history_placement=2), UNSUPPORTED,
     " keeps both halves of the history in LDS (no MI355_HISTORY_Y_IN_REGISTERS)"),
    ("hessian_from_functor", dict(hessian_from_functor=1), UNSUPPORTED,
     " is built for First-mode functions (no hessian_from_functor, hessian_diagonal or hessian_condition_stop)"),
    ("hessian_diagonal", dict(hessian_diagonal=True), UNSUPPORTED,
     " is built for First-mode functions (no hessian_from_functor, hessian_diagonal or hessian_condition_stop)"),
    ("hessian_condition_stop", dict(hessian_diagonal=True, hessian_condition_stop=10.0), UNSUPPORTED,
     " is built for First-mode functions (no hessian_from_functor, hessian_diagonal or hessian_condition_stop)"),
    ("trace", dict(trace=True), UNSUPPORTED, " records no per-iteration trace"),
    ("per_problem_data", dict(per_problem_data=True), UNSUPPORTED, " takes no per-problem data"),
    ("n", dict(n=257), UNSUPPORTED, " is built for n <= 256"),
    ("mapping", dict(lanes_per_problem=16, elems_per_lane=2), UNSUPPORTED,
     ": the mapping must cover n with 8, 16, 32 or 64 lanes at one coordinate per lane, or 64 lanes at two or four"),
    ("mapping_too_narrow", dict(lanes_per_problem=8, elems_per_lane=1), UNSUPPORTED,
     ": the mapping must cover n with 8, 16, 32 or 64 lanes at one coordinate per lane, or 64 lanes at two or four"),
]
INVALIDS = [("n", dict(n=0)), ("m_low", dict(m=0)), ("m_high", dict(m=33)), ("past", dict(past=9)), ("x0", dict(null_x0=True))]


def _raw_call(ctx, host, n=16, m=6, **change):
    """one call of the C entry with a valid Rosenbrock desc changed in the named fields; returns (code, message)"""
    import torch
    from cppnumericalsolvers_amd import capi
    lib = ctx._lib
    d = capi.Desc()
    d.objective, d.linesearch, d.n, d.m = capi.OBJ_ROSENBROCK, capi.LS_MORE_THUENTE, n, m
    d.stop = capi.default_stop()
    keep = np.ones(max(n, 1) * 4)
    keepalive = []
    for k, v in change.items():
        if k == "hessian_diagonal":
            d.hessian_diagonal = keep.ctypes.data_as(C.POINTER(C.c_double))
        elif k == "per_problem_data":
            d.per_problem_data = keep.ctypes.data
            d.per_problem_stride = 1
        elif k == "trace":
            t = capi.Trace()
            d.trace = C.addressof(t)
            keepalive.append(t)
        elif k == "past":
            d.stop.past = v
        elif k != "null_x0":
            setattr(d, k, v)
    B, nn = 4, max(d.n, 1)
    if host:
        x0 = np.zeros((B, nn), dtype=np.float32)
        x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B, dtype=np.float32)
        rc = lib.mi355_lbfgs_minimize_batch_f32_host(ctx.handle, C.byref(d), B, None if "null_x0" in change else x0.ctypes.data,
                                                     x.ctypes.data, f.ctypes.data, g.ctypes.data, None)
    else:
        x0 = torch.zeros(B, nn, dtype=torch.float32, device="cuda:0")
        x, g, f = torch.empty_like(x0), torch.empty_like(x0), torch.empty(B, dtype=torch.float32, device="cuda:0")
        rc = lib.mi355_lbfgs_minimize_batch_f32(ctx.handle, C.byref(d), B, None if "null_x0" in change else x0.data_ptr(),
                                                x.data_ptr(), f.data_ptr(), g.data_ptr(), None, None)
        torch.cuda.synchronize()
    return rc, (lib.mi355_lbfgs_last_error() or b"").decode()


def _launch_record(ctx):
    s = _amd().BatchedLbfgs(context=ctx)
    return s.last_launch(), s.last_kernel_ms()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("what,change,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(contexts, what, change, code, text, host):
    ctx = contexts[0]
    x0 = Cs._starts(16, 1)
    _device_solve(_solver(ctx, 6, None), _objective(L.ROSENBROCK), x0)   # a launch to compare the record against
    before = _launch_record(ctx)
    rc, msg = _raw_call(ctx, host, **dict(change))
    assert (rc, msg) == (code, _PREFIX + text)
    assert _launch_record(ctx) == before, "a refused call launched something"


@pytest.mark.parametrize("what,change", INVALIDS, ids=[r[0] for r in INVALIDS])
def test_invalid_arguments(contexts, what, change):
    rc, msg = _raw_call(contexts[0], False, **dict(change))
    assert rc == INVALID and msg


def test_launch_record_after_the_float_entry(contexts):
    s = _solver(contexts[0], 10, None)
    _device_solve(s, _objective(L.ROSENBROCK), Cs._starts(100, 2))
    ll = s.last_launch()
    assert (ll["lanes_per_problem"], ll["elems_per_lane"], ll["threads"]) == (64, 2, 64)
    assert ll["lds_bytes"] == (2 * 10 * 128 + 2 * 10) * 4
    assert s.last_kernel_ms() > 0.0


# ---- 7. the Python surface ---------------------------------------------------------------------------------------------------
def test_python_surface(contexts):
    import torch
    amd = _amd()
    ctx = contexts[0]
    x0 = Cs._starts(32, 11)
    s = amd.BatchedLbfgs(m=6, context=ctx, dtype=torch.float32)
    x, f, g, p = s.minimize(amd.Rosenbrock(), _dev(x0))
    torch.cuda.synchronize()
    assert x.dtype == f.dtype == g.dtype == torch.float32 and p.dtype == torch.uint8
    # the C entry, called directly
    from cppnumericalsolvers_amd import capi
    d = s._desc(amd.Rosenbrock(), 32)
    t0 = _dev(x0)
    cx, cg = torch.empty_like(t0), torch.empty_like(t0)
    cf = torch.empty(len(x0), dtype=torch.float32, device="cuda:0")
    cp = torch.empty(len(x0) * capi.PROGRESS_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    capi.check(ctx._lib.mi355_lbfgs_minimize_batch_f32(ctx.handle, C.byref(d), len(x0), t0.data_ptr(), cx.data_ptr(),
                                                       cf.data_ptr(), cg.data_ptr(), cp.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(x, cx) and torch.equal(f, cf) and torch.equal(g, cg) and torch.equal(p, cp)
    hx, hf, hg, hp = s.minimize_host(amd.Rosenbrock(), x0)
    assert hx.dtype == hf.dtype == np.float32 and hx.tobytes() == x.cpu().numpy().tobytes()
    assert hp.tobytes() == p.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        s.minimize(amd.Rosenbrock(), _dev(x0.astype(np.float64)))
    with pytest.raises(ValueError):
        s.minimize_host(amd.Rosenbrock(), x0.astype(np.float64))
    # a refusal surfaces as the existing exception type with the library's reason
    with pytest.raises(capi.EngineError, match="More-Thuente line search only"):
        amd.BatchedLbfgs(m=6, context=ctx, dtype=torch.float32, linesearch="hager_zhang").minimize(amd.Rosenbrock(), _dev(x0))
    # float64 is unchanged: the default dtype, its results, its ValueError
    d64 = amd.BatchedLbfgs(m=6, context=ctx)
    assert d64.dtype == torch.float64
    with pytest.raises(ValueError, match="float64"):
        d64.minimize(amd.Rosenbrock(), _dev(x0))
    x64 = d64.minimize(amd.Rosenbrock(), _dev(x0.astype(np.float64)))[0]
    e64 = amd.BatchedLbfgs(m=6, context=ctx, dtype=torch.float64).minimize(amd.Rosenbrock(), _dev(x0.astype(np.float64)))[0]
    torch.cuda.synchronize()
    assert x64.dtype == torch.float64 and torch.equal(x64, e64)
    for cls in (amd.BatchedBfgs, amd.BatchedLbfgsb, amd.BatchedTrustRegionNewton, amd.BatchedNewtonDescent,
                amd.BatchedGradientDescent, amd.BatchedConjugatedGradientDescent, amd.BatchedNelderMead):
        with pytest.raises(ValueError, match="float64 only"):
            cls(context=ctx, dtype=torch.float32)
        cls(context=ctx, dtype=torch.float64)


# ---- 8. the C++ drop-in ------------------------------------------------------------------------------------------------------
def test_cpp_header_native_float(contexts):
    """tests/lbfgs_f32/f32_header_test (prebuilt by build()): Lbfgs<RosenbrockF, 6> with SetNativeFloat(true) from the two
    starts of verify.cc, through Minimize and MinimizeBatch, is the twin bit for bit; without the setter the same program
    takes the widened fp64 path."""
    import os
    import subprocess
    import torch
    out = subprocess.run([os.path.join(L.L32_DIR, "_build", "f32_header_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr

    def parse(tag):
        rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith(tag + " ")]
        assert len(rows) == 2, out.stdout
        u = lambda *h: np.array([int(v, 16) for v in h], dtype=np.uint32).view(np.float32)
        return [dict(x=u(r[2], r[3]), f=u(r[5]), g=u(r[7], r[8]), status=int(r[10]), iterations=int(r[12]),
                     x_delta=u(r[14]), f_delta=u(r[16]), gradient_norm=u(r[18])) for r in rows]

    def same(rows, x, f, g, prog, what):
        for b, r in enumerate(rows):
            assert r["x"].tobytes() == x[b].tobytes() and r["f"].tobytes() == f[b:b + 1].tobytes(), what
            assert r["g"].tobytes() == g[b].tobytes(), what
            assert (r["status"], r["iterations"]) == (prog["status"][b], prog["num_iterations"][b]), what
            for fld in ("x_delta", "f_delta", "gradient_norm"):
                assert r[fld].tobytes() == prog[fld][b:b + 1].astype(np.float32).tobytes(), what + " " + fld

    twin = L.twin_solve(L.ROSENBROCK, 6, Cs.VERIFY_STARTS, order=L.DEVICE_ORDER)
    same(parse("minimize"), *twin, "Minimize")
    same(parse("batch"), *twin, "MinimizeBatch")
    # without the setter: the fp64 engine on the widened starts (thresholds: the float presets widened), rounded to float
    amd = _amd()
    stop = amd.capi.default_stop()
    for fld in ("x_delta", "f_delta", "gradient_norm", "past_delta"):
        setattr(stop, fld, float(np.float32(getattr(stop, fld))))
    s = amd.BatchedLbfgs(m=6, stopping_progress=stop, context=contexts[0], arithmetic="exact")
    x, f, g, p = s.minimize(amd.Rosenbrock(), _dev(Cs.VERIFY_STARTS.astype(np.float64)))
    torch.cuda.synchronize()
    same(parse("widened"), x.cpu().numpy().astype(np.float32), f.cpu().numpy().astype(np.float32),
         g.cpu().numpy().astype(np.float32), amd.progress_to_numpy(p), "widened")
