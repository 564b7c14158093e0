"""The float ask/tell L-BFGS on the device: mi355_lbfgs_ask_tell_f32_*, amd.LbfgsAskTell on a float32 solver,
BatchedLbfgs(dtype=torch.float32).minimize_callable and the C++ header's LbfgsAskTellF32.

The yardstick is always the persistent float kernel (BatchedLbfgs(dtype=torch.float32, arithmetic="exact").minimize) on
the same device batch, with the library's float evaluation entry (solver.evaluate) as the callback; equality is bitwise
on x, f, g and on every field of the progress record.
5. Rosenbrock and DiagQuadratic over dimensions, histories and stopping records.
6. Every mapping, a grid capped at one workgroup, check_every = 7, a non-default stream, hostile starts, poisoned rows.
7. A value-only float32 objective in torch ops with per-problem data reaches its closed-form minimiser.
8. Every refusal returns its code and names its reason, and launches nothing; mismatched dtypes; max_rounds.
9. The C++ header test binary reproduces the persistent float kernel's bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import at32_lib
import at_lib
import l32_cases as Cs
import l32_lib as L

pytestmark = pytest.mark.gpu
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
B = at32_lib.B


def _amd():
    import cppnumericalsolvers_amd as amd
    return amd


@pytest.fixture(scope="module")
def context():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ctx = _amd().Context(0)
    yield ctx
    ctx.close()


def _solver(ctx, m=6, stop=None, **kw):
    import torch
    stop = at32_lib.capi_stop(stop if stop is not None else L.default_stop())
    return _amd().BatchedLbfgs(m=m, stopping_progress=stop, context=ctx, arithmetic="exact", dtype=torch.float32, **kw)


def _objective(objective, n):
    amd = _amd()
    if objective == "rosenbrock":
        return amd.Rosenbrock()
    p = at_lib.diag_params(n)
    return amd.DiagQuadratic(p[:n], float(p[n]))


def _host(out):
    import torch
    torch.cuda.synchronize()
    x, f, g, p = out
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), _amd().progress_to_numpy(p)


def _both(solver, objective, x0, **kw):
    """(ask/tell with the library's float evaluation entry as the callback, persistent float kernel, rounds)"""
    import torch
    x0d = torch.from_numpy(x0).to(solver.device)
    want = _host(solver.minimize(objective, x0d))
    rounds = [0]

    def fn(X):
        assert X.dtype == torch.float32
        rounds[0] += 1
        return solver.evaluate(objective, X)

    got = _host(solver.minimize_callable(fn, x0d, **kw))
    return got, want, rounds[0]


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 6])
@pytest.mark.parametrize("n", [2, 13, 33, 65, 130])
@pytest.mark.parametrize("objective", ["rosenbrock", "diag_quadratic"])
def test_callback_of_the_librarys_float_evaluation_is_the_persistent_float_kernel(context, objective, n, m):
    x0 = at32_lib.starts(objective, B, n, seed=1000 * n + m)
    got, want, rounds = _both(_solver(context, m=m), _objective(objective, n), x0)
    at32_lib.assert_same(got, want, "ask/tell f32 vs persistent float kernel: %s n=%d m=%d" % (objective, n, m))
    assert rounds >= int(want[3]["nfev"].max())
    assert np.all(want[3]["status"] > 0)


@pytest.mark.parametrize("name", ["default", "conservative", "past0", "iters1", "iters3", "zero40"])
def test_stopping_records(context, name):
    fields = Cs.STOPS[name]
    x0 = at32_lib.starts("rosenbrock", B, 13, seed=31)
    got, want, rounds = _both(_solver(context, stop=L.make_stop(**fields)), _amd().Rosenbrock(), x0)
    at32_lib.assert_same(got, want, name)
    assert rounds >= int(want[3]["nfev"].max())
    if name == "iters1":   # (the limit fires when the count exceeds it: progress.h:212)
        assert np.all(want[3]["num_iterations"] <= 2) and np.any(want[3]["status"] == 1), want[3]["status"]
    if name in ("default", "conservative"):
        assert fields["past"] > 0


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,E", at32_lib.MAPPINGS)
@pytest.mark.parametrize("n", [13, 130])
def test_every_built_mapping(context, n, W, E):
    import torch
    amd = _amd()
    solver = _solver(context, lanes_per_problem=W, elems_per_lane=E)
    if W * E < n:
        with pytest.raises(amd.capi.EngineError) as e:
            amd.LbfgsAskTell(solver, torch.zeros(2, n, dtype=torch.float32, device=solver.device))
        assert e.value.code == amd.capi.ERR_UNSUPPORTED and "mapping" in str(e.value)
        assert str(e.value).count("Lbfgs ask/tell f32") == 1
        return
    x0 = at32_lib.starts("rosenbrock", B, n, seed=77)
    got, want, _ = _both(solver, amd.Rosenbrock(), x0)
    at32_lib.assert_same(got, want, "n=%d %dx%d" % (n, W, E))
    ll = solver.last_launch()
    assert (ll["lanes_per_problem"], ll["elems_per_lane"]) == (W, E)


VARIATION = dict(n=33, m=6, seed=909)


def _variation_x0():
    return at32_lib.starts("rosenbrock", B, VARIATION["n"], seed=VARIATION["seed"])


def test_capped_grid_of_one_workgroup(monkeypatch, context):
    """one workgroup strides over all 131 problems"""
    amd = _amd()
    x0 = _variation_x0()
    _, want, _ = _both(_solver(context), amd.Rosenbrock(), x0)
    monkeypatch.setenv(CAP_ENV, "1")
    ctx = amd.Context(0)
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        solver = _solver(ctx)
        got, _, _ = _both(solver, amd.Rosenbrock(), x0)
        assert solver.last_launch()["blocks"] == 1
    finally:
        ctx.close()
    at32_lib.assert_same(got, want, "one workgroup")


def test_check_every_7(context):
    """the count is read every seventh round: up to six rounds run on a finished batch and change nothing"""
    amd = _amd()
    x0 = _variation_x0()
    solver = _solver(context)
    got, want, rounds = _both(solver, amd.Rosenbrock(), x0, check_every=7)
    at32_lib.assert_same(got, want, "check_every=7")
    assert rounds % 7 == 0
    got1, _, rounds1 = _both(solver, amd.Rosenbrock(), x0)
    at32_lib.assert_same(got1, want, "check_every=1")
    assert rounds1 <= rounds < rounds1 + 7


def test_non_default_stream(context):
    import torch
    amd = _amd()
    x0 = _variation_x0()
    solver = _solver(context)
    _, want, _ = _both(solver, amd.Rosenbrock(), x0)
    stream = torch.cuda.Stream(device=solver.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got, _, _ = _both(solver, amd.Rosenbrock(), x0)
    at32_lib.assert_same(got, want, "non-default stream")


@pytest.mark.parametrize("n", [5, 65])
def test_hostile_starts(context, n):
    """NaN / inf coordinates, overflowing magnitudes, rows already at the minimiser: the bail-out and the refused-search
    phase.  Every NaN of either path is the canonical quiet NaN, so the comparison stays bitwise."""
    x0 = np.concatenate([at32_lib.hostile_starts(n), at32_lib.starts("rosenbrock", 4, n, seed=3)])
    stop = L.make_stop(**{**L.STOP_PRESETS["default"], "num_iterations": 40})
    got, want, _ = _both(_solver(context, stop=stop), _amd().Rosenbrock(), x0)
    at32_lib.assert_same(got, want, "hostile starts, n=%d" % n)
    at_minimiser = want[3][-7:-4]
    assert np.all(at_minimiser["nfev"] == 1), at_minimiser   # the search was refused: no evaluation but the first


def test_handle_protocol_and_poisoned_rows(context):
    """LbfgsAskTell by hand on a float32 solver: .x is a float32 view of the library's buffer, results() at any time, the
    rows of finished and of no-evaluation problems are never read (NaN is handed back for them), extra rounds change
    nothing."""
    import torch
    amd = _amd()
    n = 5
    x0 = np.concatenate([at32_lib.starts("rosenbrock", B - 3, n, seed=11), np.ones((3, n), dtype=np.float32)])
    solver = _solver(context)
    x0d = torch.from_numpy(x0).to(solver.device)
    want = _host(solver.minimize(amd.Rosenbrock(), x0d))
    with amd.LbfgsAskTell(solver, x0d) as at:
        assert at.x.shape == (B, n) and at.x.dtype == torch.float32 and at.x.data_ptr() != x0d.data_ptr()
        ptr = at.x.data_ptr()
        assert torch.equal(at.x, x0d) and at.active == B
        first = _host(at.results())
        assert first[0].dtype == np.float32 and np.array_equal(first[0], x0) and np.all(first[3]["status"] == -1)
        active, rounds = B, 0
        while active > 0:
            f, g = solver.evaluate(amd.Rosenbrock(), at.x)
            assert f.dtype == torch.float32 and g.dtype == torch.float32
            # finished problems; and the three rows at the minimiser, whose search is refused in the first round (g = 0):
            # they ask for no evaluation in the second round and have finished after it
            unread = _host(at.results())[3]["status"] > 0
            if rounds >= 1:
                unread[-3:] = True
            rows = torch.from_numpy(unread).to(solver.device)
            f[rows] = float("nan")
            g[rows] = float("nan")
            active = at.tell(f, g)
            rounds += 1
            assert active == at.active and at.x.data_ptr() == ptr
            assert rounds < 5000
        for _ in range(3):   # a finished batch stays as it is
            assert at.tell(torch.full_like(f, float("nan")), torch.full_like(g, float("nan"))) == 0
        got = _host(at.results())
        assert np.array_equal(at.x.cpu().numpy(), got[0])   # the evaluation buffer holds the returned x
    at.close()
    at32_lib.assert_same(got, want, "by hand, NaN rows for finished and no-evaluation problems")
    with pytest.raises(RuntimeError):
        at.tell(f, g)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
def test_value_only_torch_objective_in_float32(context):
    """f_b(x) = 1/2 sum_i a_i (x_i - c_{b,i})^2 in float32 torch ops, the gradient from autograd, under the absolute
    gradient test tau = 1e-4 alone (and 200 iterations).  g_i = a_i (x_i - c_i) up to two float roundings of 2^-24 each,
    so |x_i - c_i| <= tau / a_i (1 + 2^-23)^2 < 2 tau / a_min; the gradient's granularity a ulp(2) ~ 5e-7 is far below
    tau.  tests/test_ask_tell_f32_cpu.py clears these inputs on the float twin."""
    import torch
    a, c, x0 = at32_lib.quadratic_inputs()
    tau = at32_lib.QUAD_TAU
    solver = _solver(context, m=at32_lib.QUAD_M, stop=L.make_stop(**at32_lib.quadratic_stop_fields()))
    ad, cd = torch.from_numpy(a).to(solver.device), torch.from_numpy(c).to(solver.device)
    seen = []

    def value(X):
        seen.append(X.dtype)
        r = X - cd
        return 0.5 * (ad * r * r).sum(dim=1)

    x, f, g, p = _host(solver.minimize_callable(value, torch.from_numpy(x0).to(solver.device), max_rounds=2000))
    assert set(seen) == {torch.float32} and x.dtype == f.dtype == g.dtype == np.float32
    err = float(np.abs(x.astype(np.float64) - c.astype(np.float64)).max())
    print("status %s, gradient_norm <= %.3g, |x - c|_inf = %.3g (bound %.3g), iterations <= %d, evaluations <= %d"
          % (np.unique(p["status"]).tolist(), p["gradient_norm"].max(), err, 2 * tau / float(a.min()),
             p["num_iterations"].max(), p["nfev"].max()))
    assert np.all(p["status"] == at32_lib.GRADIENT_STATUS), np.unique(p["status"], return_counts=True)
    assert p["gradient_norm"].max() <= tau
    assert err <= 2 * tau / float(a.min())


# ---- 8 ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_launch_nothing():
    import torch
    amd = _amd()
    from cppnumericalsolvers_amd import capi
    ctx = amd.Context(0)
    try:
        lib = ctx._lib
        x0 = torch.zeros(4, 8, dtype=torch.float32, device="cuda:0")

        def desc(**over):
            d = capi.Desc()
            d.objective, d.linesearch, d.n, d.m = capi.OBJ_ROSENBROCK, capi.LS_MORE_THUENTE, 8, 6
            d.stop = capi.default_stop()
            for k, v in over.items():
                setattr(d, k, v)
            return d

        diag = np.ones(8)
        trace = amd.Trace([0], 4, 8, "cuda:0")
        unsupported = [
            (desc(linesearch=capi.LS_HAGER_ZHANG), "Hager-Zhang"),
            (desc(arithmetic=capi.ARITH_FMA), "MI355_ARITH_FMA"),
            (desc(history_placement=capi.HISTORY_Y_IN_REGISTERS), "MI355_HISTORY_Y_IN_REGISTERS"),
            (desc(hessian_from_functor=1), "hessian_from_functor"),
            (desc(hessian_diagonal=diag.ctypes.data_as(C.POINTER(C.c_double))), "hessian_diagonal"),
            (desc(hessian_condition_stop=10.0), "hessian_condition_stop"),
            (desc(trace=trace.c_pointer()), "trace"),
            (desc(per_problem_data=x0.data_ptr(), per_problem_stride=8), "per_problem_data"),
            (desc(n=257), "n <= 256"),
            (desc(m=33), "MI355_LBFGS_MAX_M"),
            (desc(lanes_per_problem=16, elems_per_lane=2), "mapping"),
            (desc(lanes_per_problem=4, elems_per_lane=2), "mapping"),
            (desc(n=13, lanes_per_problem=8, elems_per_lane=1), "mapping"),
        ]
        for d, text in unsupported:
            h = C.c_void_p()
            rc = lib.mi355_lbfgs_ask_tell_f32_create(ctx.handle, C.byref(d), 4, x0.data_ptr(), None, C.byref(h))
            message = lib.mi355_lbfgs_last_error().decode()
            assert rc == capi.ERR_UNSUPPORTED and not h.value, (text, rc, message)
            assert message.startswith("Lbfgs ask/tell f32") and text in message, (text, message)
        # validate()'s argument errors stay argument errors; so do null arguments
        for d, text in ((desc(m=0), "m out of range"), (desc(n=0), "n out of range"), (desc(arithmetic=7), "arithmetic")):
            h = C.c_void_p()
            rc = lib.mi355_lbfgs_ask_tell_f32_create(ctx.handle, C.byref(d), 4, x0.data_ptr(), None, C.byref(h))
            assert rc == capi.ERR_INVALID_ARGUMENT and text in lib.mi355_lbfgs_last_error().decode() and not h.value
        h = C.c_void_p()
        assert lib.mi355_lbfgs_ask_tell_f32_create(ctx.handle, C.byref(desc()), 4, None, None, C.byref(h)) == \
            capi.ERR_INVALID_ARGUMENT and not h.value
        # the objective and its parameter fields are not read; B = 0 is valid
        d = desc(objective=4242, n_params=3)
        capi.check(lib.mi355_lbfgs_ask_tell_f32_create(ctx.handle, C.byref(d), 4, x0.data_ptr(), None, C.byref(h)))
        assert lib.mi355_lbfgs_ask_tell_f32_step(h, None, None, None, None) == capi.ERR_INVALID_ARGUMENT
        capi.check(lib.mi355_lbfgs_ask_tell_f32_destroy(h))
        h = C.c_void_p()
        capi.check(lib.mi355_lbfgs_ask_tell_f32_create(ctx.handle, C.byref(desc()), 0, None, None, C.byref(h)))
        count = C.c_int64(-1)
        capi.check(lib.mi355_lbfgs_ask_tell_f32_step(h, None, None, C.byref(count), None))
        assert count.value == 0
        capi.check(lib.mi355_lbfgs_ask_tell_f32_results(h, None, None, None, None, None))
        capi.check(lib.mi355_lbfgs_ask_tell_f32_destroy(h))
        v = [C.c_int32(-1) for _ in range(6)]
        capi.check(lib.mi355_lbfgs_last_launch(ctx.handle, *[C.byref(t) for t in v]))
        assert [t.value for t in v] == [0] * 6, "a refused (or merely created) solve launched a solve kernel"
    finally:
        ctx.close()


def test_mismatched_dtypes_and_refused_options(context):
    import torch
    amd = _amd()
    f32 = _solver(context)
    f64 = amd.BatchedLbfgs(m=6, context=context, arithmetic="exact")
    x32 = torch.zeros(4, 8, dtype=torch.float32, device=f32.device)
    x64 = x32.double()
    with pytest.raises(ValueError, match="float32"):
        amd.LbfgsAskTell(f32, x64)
    with pytest.raises(ValueError, match="float64"):
        amd.LbfgsAskTell(f64, x32)
    with pytest.raises(ValueError):
        f32.minimize_callable(lambda X: (X.sum(dim=1), torch.ones_like(X)), x64)
    for solver, x0, other in ((f32, x32, torch.float64), (f64, x64, torch.float32)):
        with amd.LbfgsAskTell(solver, x0) as at:
            f, g = torch.zeros(4, dtype=x0.dtype, device=x0.device), torch.zeros_like(x0)
            with pytest.raises(ValueError):
                at.tell(f.to(other), g)
            with pytest.raises(ValueError):
                at.tell(f, g.to(other))
            assert at.active == 4   # nothing ran
    # a float32 solver configured with what the path does not build raises the library's message
    for kw, text in ((dict(linesearch="hager_zhang"), "Hager-Zhang"), (dict(history_placement=2), "MI355_HISTORY_Y_IN_REGISTERS"),
                     (dict(condition_hessian=5.0), "hessian_condition_stop")):
        solver = amd.BatchedLbfgs(m=6, context=context, dtype=torch.float32, **kw)
        with pytest.raises(amd.capi.EngineError) as e:
            solver.minimize_callable(lambda X: (X.sum(dim=1), torch.ones_like(X)), x32)
        assert e.value.code == amd.capi.ERR_UNSUPPORTED and text in str(e.value), str(e.value)
    # the other solvers stay float64 only
    with pytest.raises(ValueError):
        amd.BatchedLbfgsb(context=context, dtype=torch.float32)
    with pytest.raises(TypeError):
        amd.LbfgsAskTell(amd.BatchedBfgs(context=context), x64)


def test_max_rounds_exceeded_raises(context):
    import torch
    amd = _amd()
    solver = _solver(context)
    x0d = torch.from_numpy(at32_lib.starts("rosenbrock", 9, 8, seed=1)).to(solver.device)
    with pytest.raises(RuntimeError, match="still active after max_rounds = 3"):
        solver.minimize_callable(lambda X: solver.evaluate(amd.Rosenbrock(), X), x0d, max_rounds=3)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["atf_header_test", "atf_header_test_noexcept"])
def test_cpp_header_binary_matches_the_persistent_float_kernel(context, binary):
    import torch
    amd = _amd()
    path = os.path.join(at32_lib.HEADER_DIR, "_build", binary)
    assert os.access(path, os.X_OK), "%s is not built (run __graft_entry__.build())" % path
    out = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    n, m, Bc = 13, 6, 5
    x0 = np.array([[(1.0 if j % 2 else -1.25) + 0.0625 * b for j in range(n)] for b in range(Bc)], dtype=np.float32)
    solver = _solver(context, m=m)
    x, f, g, p = _host(solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to(solver.device)))

    def hex64(a):
        return [format(int(v), "016x") for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]

    def hex32(a):
        assert np.asarray(a).dtype == np.float32
        return [format(int(v), "08x") for v in np.ascontiguousarray(a).reshape(-1).view(np.uint32)]

    lines = out.stdout.splitlines()
    assert sum(line.startswith("rounds ") for line in lines) == 2
    for tag in ("handle", "call"):
        rows = [line.split() for line in lines if line.startswith(tag + " ")]
        assert len(rows) == Bc, out.stdout
        for b, w in enumerate(rows):
            want = ([tag, str(b), "status", str(p["status"][b]), "iterations", str(p["num_iterations"][b]), "nfev",
                     str(p["nfev"][b]), "sum_k", str(p["sum_k"][b]), "x_delta"] + hex64(p["x_delta"][b]) + ["f_delta"] +
                    hex64(p["f_delta"][b]) + ["gradient_norm"] + hex64(p["gradient_norm"][b]) + ["f"] + hex32(f[b]) +
                    ["x"] + hex32(x[b]) + ["g"] + hex32(g[b]))
            assert w == want, (tag, b)
    if binary == "atf_header_test":
        mis = subprocess.run([path, "--misuse"], capture_output=True, text=True, timeout=120)
        assert mis.returncode == 0 and mis.stdout.startswith("ok: Hager-Zhang"), mis.stdout + mis.stderr
