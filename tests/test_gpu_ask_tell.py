"""The ask/tell (reverse communication) L-BFGS on the device: mi355_lbfgs_ask_tell_*, amd.LbfgsAskTell,
BatchedLbfgs.minimize_callable and the C++ header.

1. Fed the library's own evaluation entry as the callback, minimize_callable returns the bits of the persistent exact kernel
   (x, f, g and every progress field, on every problem).
2. The same results are the CPU twin's in butterfly order (tests/ask_tell/at_twin.hpp), hostile starts included.
3. An objective written in torch ops lands within 1e-6 of the persistent kernel on the inputs tests/test_ask_tell_twin.py
   cleared, with the same status wherever the twin's two orders agree.
4. A value-only torch objective with per-problem data, differentiated by autograd, reaches the closed-form minimiser.
5. Every refusal returns its code and names its reason, and launches nothing.
6. The C++ header test binary reproduces the persistent kernel too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import at_lib
import oracle_lib

pytestmark = pytest.mark.gpu
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
B = 131
MAPPINGS = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))
GRADIENT_STATUS = 4


def _objective(amd, objective, n):
    if objective == "rosenbrock":
        return amd.Rosenbrock()
    p = at_lib.diag_params(n)
    return amd.DiagQuadratic(p[:n], float(p[n]))


def _stop(stop):
    """an oracle_lib.Stop as the engine's capi.Stop (the same fields)"""
    from cppnumericalsolvers_amd import capi
    s = capi.Stop()
    for name, _ in capi.Stop._fields_:
        setattr(s, name, getattr(stop, name))
    return s


def _host(amd, out):
    import torch
    torch.cuda.synchronize()
    x, f, g, p = out
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


def _both(amd, solver, objective, x0, **kw):
    """(persistent kernel, ask/tell with the library's evaluation entry as the callback) on the same device batch"""
    import torch
    x0d = torch.from_numpy(x0).to(solver.device)
    want = _host(amd, solver.minimize(objective, x0d))
    rounds = [0]

    def fn(X):
        rounds[0] += 1
        return solver.evaluate(objective, X)

    got = _host(amd, solver.minimize_callable(fn, x0d, **kw))
    return got, want, rounds[0]


@pytest.mark.parametrize("m", at_lib.HISTORIES)
@pytest.mark.parametrize("n", at_lib.DIMS)
@pytest.mark.parametrize("objective", ["rosenbrock", "diag_quadratic"])
def test_callback_of_the_librarys_own_evaluation_is_the_persistent_kernel_and_the_twin(gpu_solver_factory, objective, n, m):
    import cppnumericalsolvers_amd as amd
    stop = at_lib.base_stop()
    x0 = at_lib.starts(objective, B, n, seed=1000 * n + m)
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    got, want, rounds = _both(amd, solver, _objective(amd, objective, n), x0)
    at_lib.assert_same_results(got, want, "ask/tell vs persistent kernel: %s n=%d m=%d" % (objective, n, m))
    assert rounds >= int(want[3]["nfev"].max())
    twin = at_lib.twin_minimize_driven(objective, x0, m, stop, params=at_lib.params_of(objective, n))
    at_lib.assert_same_results(got, twin, "ask/tell vs twin: %s n=%d m=%d" % (objective, n, m))
    assert rounds == twin[4]


@pytest.mark.parametrize("W,E", MAPPINGS)
@pytest.mark.parametrize("n", [13, 130])
def test_every_built_mapping(gpu_solver_factory, n, W, E):
    import cppnumericalsolvers_amd as amd
    if W * E < n:
        solver = gpu_solver_factory(m=6, lanes_per_problem=W, elems_per_lane=E)
        import torch
        with pytest.raises(amd.capi.EngineError) as e:
            amd.LbfgsAskTell(solver, torch.zeros(2, n, dtype=torch.float64, device=solver.device))
        assert e.value.code == amd.capi.ERR_UNSUPPORTED and "mapping" in str(e.value)
        return
    stop = at_lib.base_stop()
    x0 = at_lib.starts("rosenbrock", B, n, seed=77)
    solver = gpu_solver_factory(m=6, stopping_progress=_stop(stop), lanes_per_problem=W, elems_per_lane=E)
    got, want, rounds = _both(amd, solver, amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got, want, "n=%d %dx%d" % (n, W, E))
    ll = solver.last_launch()
    assert (ll["lanes_per_problem"], ll["elems_per_lane"]) == (W, E)
    twin = at_lib.twin_minimize_driven("rosenbrock", x0, 6, stop, width=W * E)
    at_lib.assert_same_results(got, twin, "twin n=%d %dx%d" % (n, W, E))


@pytest.mark.parametrize("name", ["past8", "everything_off_but_limit", "x_delta_needs_3", "f_delta_rel"])
def test_stopping_records(gpu_solver_factory, name):
    import cppnumericalsolvers_amd as amd
    stop = at_lib.stop_records()[name]
    x0 = at_lib.starts("rosenbrock", B, 13, seed=31)
    solver = gpu_solver_factory(m=6, stopping_progress=_stop(stop))
    got, want, _ = _both(amd, solver, amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got, want, name)
    at_lib.assert_same_results(got, at_lib.twin_minimize_driven("rosenbrock", x0, 6, stop), "twin " + name)


VARIATION = dict(objective="rosenbrock", n=33, m=6, seed=909)


def _variation_inputs():
    v = VARIATION
    return at_lib.starts(v["objective"], B, v["n"], seed=v["seed"]), at_lib.base_stop()


def test_check_every_7(gpu_solver_factory):
    """the count is read every seventh round: up to six rounds run on a finished batch and change nothing"""
    import cppnumericalsolvers_amd as amd
    x0, stop = _variation_inputs()
    solver = gpu_solver_factory(m=VARIATION["m"], stopping_progress=_stop(stop))
    got, want, rounds = _both(amd, solver, amd.Rosenbrock(), x0, check_every=7)
    at_lib.assert_same_results(got, want, "check_every=7")
    assert rounds % 7 == 0
    got1, _, rounds1 = _both(amd, solver, amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got1, want, "check_every=1")
    assert rounds1 <= rounds < rounds1 + 7


def test_non_default_stream(gpu_solver_factory):
    import torch
    import cppnumericalsolvers_amd as amd
    x0, stop = _variation_inputs()
    solver = gpu_solver_factory(m=VARIATION["m"], stopping_progress=_stop(stop))
    _, want, _ = _both(amd, solver, amd.Rosenbrock(), x0)
    stream = torch.cuda.Stream(device=solver.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got, _, _ = _both(amd, solver, amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got, want, "non-default stream")


def test_capped_grid_of_one_workgroup(monkeypatch, gpu_solver_factory):
    """one workgroup strides over all 131 problems (gpu_solver_factory is asked for first, so that the session's shared
    context is never created under the cap)"""
    import cppnumericalsolvers_amd as amd
    x0, stop = _variation_inputs()
    _, want, _ = _both(amd, gpu_solver_factory(m=VARIATION["m"], stopping_progress=_stop(stop)), amd.Rosenbrock(), x0)
    monkeypatch.setenv(CAP_ENV, "1")
    ctx = amd.Context(0)
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        solver = amd.BatchedLbfgs(m=VARIATION["m"], stopping_progress=_stop(stop), arithmetic="exact", context=ctx)
        got, _, _ = _both(amd, solver, amd.Rosenbrock(), x0)
        assert solver.last_launch()["blocks"] == 1
    finally:
        ctx.close()
    at_lib.assert_same_results(got, want, "one workgroup")


@pytest.mark.parametrize("objective,n", [("rosenbrock", 5), ("rosenbrock", 65), ("diag_quadratic", 13)])
def test_hostile_starts_equal_the_twin(gpu_solver_factory, objective, n):
    """NaN / inf coordinates, overflowing magnitudes: the bail-out and the refused-search phase.  The callback is the
    library's evaluation entry; the twin evaluates with the oracle's functor in the same order."""
    import cppnumericalsolvers_amd as amd
    stop = at_lib.base_stop(num_iterations=40)
    x0 = np.concatenate([oracle_lib.hostile_starts(n), np.ones((3, n)), at_lib.starts(objective, 4, n, seed=3)])
    solver = gpu_solver_factory(m=6, stopping_progress=_stop(stop))
    got, want, _ = _both(amd, solver, _objective(amd, objective, n), x0)
    twin = at_lib.twin_minimize_driven(objective, x0, 6, stop, params=at_lib.params_of(objective, n))
    at_lib.assert_same_results(got, twin, "hostile starts vs twin", nan_equal=True)
    at_lib.assert_same_results(got, want, "hostile starts vs persistent kernel")


def test_handle_protocol_and_poisoned_rows(gpu_solver_factory):
    """LbfgsAskTell by hand: .x is a view of the library's buffer (no copy), results() at any time, the rows of finished
    problems are never read (NaN is handed back for them), extra rounds change nothing, close() is idempotent."""
    import torch
    import cppnumericalsolvers_amd as amd
    x0, stop = _variation_inputs()
    solver = gpu_solver_factory(m=VARIATION["m"], stopping_progress=_stop(stop))
    x0d = torch.from_numpy(x0).to(solver.device)
    want = _host(amd, solver.minimize(amd.Rosenbrock(), x0d))
    with amd.LbfgsAskTell(solver, x0d) as at:
        assert at.x.shape == (B, 33) and at.x.dtype == torch.float64 and at.x.data_ptr() != x0d.data_ptr()
        ptr = at.x.data_ptr()
        assert torch.equal(at.x, x0d) and at.active == B
        first = _host(amd, at.results())
        assert np.array_equal(first[0], x0) and np.all(first[3]["status"] == -1)
        active, rounds = B, 0
        while active > 0:
            f, g = solver.evaluate(amd.Rosenbrock(), at.x)
            done = torch.from_numpy(_host(amd, at.results())[3]["status"] > 0).to(solver.device)
            f[done] = float("nan")
            g[done] = float("nan")
            active = at.tell(f, g)
            rounds += 1
            assert active == at.active and at.x.data_ptr() == ptr
            assert rounds < 2000
        for _ in range(3):   # a finished batch stays as it is
            assert at.tell(torch.full_like(f, float("nan")), torch.full_like(g, float("nan"))) == 0
        got = _host(amd, at.results())
        assert np.array_equal(at.x.cpu().numpy(), got[0])   # the evaluation buffer holds the returned x
    at.close()
    at_lib.assert_same_results(got, want, "by hand, NaN rows for finished problems")
    with pytest.raises(RuntimeError):
        at.tell(f, g)


# ---- 3. an objective written in torch ops ----------------------------------------------------------------------------------
def _torch_objective(objective, n, device):
    import torch
    if objective == "rosenbrock":
        def fn(X):
            a, b = X[:, :-1], X[:, 1:]
            t1, t2 = 1.0 - a, b - a * a
            f = (t1 * t1 + 100.0 * t2 * t2).sum(dim=1)
            g = torch.zeros_like(X)
            g[:, :-1] = -2.0 * t1 - 400.0 * t2 * a
            g[:, 1:] += 200.0 * t2
            return f, g
        return fn
    p = at_lib.diag_params(n)
    a, c = torch.from_numpy(p[:n]).to(device), float(p[n])

    def fn(X):
        return (a * X * X).sum(dim=1) + c, 2.0 * a * X
    return fn


@pytest.mark.parametrize("objective,n,m", at_lib.TORCH_CASES)
def test_objective_written_in_torch_ops(gpu_solver_factory, objective, n, m):
    import torch
    import cppnumericalsolvers_amd as amd
    stop = at_lib.torch_case_stop()
    x0 = at_lib.torch_case_inputs(objective, n)
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    x0d = torch.from_numpy(x0).to(solver.device)
    want = _host(amd, solver.minimize(_objective(amd, objective, n), x0d))
    got = _host(amd, solver.minimize_callable(_torch_objective(objective, n, solver.device), x0d, max_rounds=5000))
    dx = float(np.max(np.abs(got[0] - want[0])))
    df = float(np.max(np.abs(got[1] - want[1])))
    params = at_lib.params_of(objective, n)
    seq = oracle_lib.minimize_batch(objective, x0, m=m, stop=stop, params=params, reduction="sequential")
    but = oracle_lib.minimize_batch(objective, x0, m=m, stop=stop, params=params, reduction="butterfly",
                                    width=at_lib.padded_width(n))
    agree = seq[3]["status"] == but[3]["status"]
    print("torch-op %s n=%d m=%d: max|dx| %.3g max|df| %.3g vs the persistent kernel; twin orders agree on %d of %d"
          % (objective, n, m, dx, df, int(agree.sum()), len(x0)))
    assert int((~agree).sum()) <= at_lib.MAX_STATUS_DISAGREEMENT * len(x0)
    assert dx <= at_lib.CONTRACT and df <= at_lib.CONTRACT
    assert np.array_equal(got[3]["status"][agree], want[3]["status"][agree])


# ---- 4. value-only, autograd, per-problem data --------------------------------------------------------------------------------
def test_value_only_objective_with_per_problem_data(gpu_solver_factory):
    """f_b(x) = 1/2 ||A_b x - y_b||^2 + 1/2 lambda ||x||^2, A_b 12 x 5: H = A^T A + lambda I >= lambda I, so
    ||x - x*|| <= ||g(x)|| / lambda for every x (g(x) = H (x - x*)).
    The right-hand sides are 0.01 N(0, 1), so that f* is about 7e-4.  A More-Thuente search accepts a step on the
    DECREASE of f, which near the minimiser is about ||g||^2 / (2 lambda_max(H)), lambda_max about 25: 4e-16 at
    ||g|| = 1e-7 and 4e-18 at the gradient stop of 1e-8.  With y = N(0, 1) f* is about 7 and one ulp of it is 9e-16: the
    last decade of the gradient lies below what fp64 resolves in f, and the reference's own algorithm stalls there (the
    CPU oracle on the same data in its reference order: 30 of 257 problems run 16 trials per iteration to the iteration
    limit).  At f* = 7e-4 one ulp is 1e-19 and every decrease down to the stop is resolved."""
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    Bv, rows, n, lam = 257, 12, 5, 0.1
    rng = np.random.default_rng(20261019)
    A, y = rng.normal(size=(Bv, rows, n)), 0.01 * rng.normal(size=(Bv, rows))
    stop = capi.default_stop()
    stop.num_iterations, stop.x_delta, stop.f_delta, stop.past = 500, 0.0, 0.0, 0
    stop.gradient_norm, stop.gradient_norm_relative = 1e-8, 0
    solver = gpu_solver_factory(m=10, stopping_progress=stop)
    Ad, yd = torch.from_numpy(A).to(solver.device), torch.from_numpy(y).to(solver.device)

    def value(X):
        r = torch.einsum("brn,bn->br", Ad, X) - yd
        return 0.5 * (r * r).sum(dim=1) + 0.5 * lam * (X * X).sum(dim=1)

    x, f, g, p = _host(amd, solver.minimize_callable(value, torch.zeros(Bv, n, dtype=torch.float64, device=solver.device),
                                                     max_rounds=2000))
    assert np.all(p["status"] == GRADIENT_STATUS), np.unique(p["status"], return_counts=True)
    # the check's own arithmetic in extended precision (x86 long double), so that its rounding (1e-19 relative) stays far
    # below the 1e-6 relative slack of the bound even where the solver lands on ||g|| ~ 1e-12
    ld = np.longdouble
    Al, yl, xl = A.astype(ld), y.astype(ld), x.astype(ld)
    H = np.einsum("brn,brk->bnk", Al, Al) + ld(lam) * np.eye(n, dtype=ld)
    c = np.einsum("brn,br->bn", Al, yl)
    gx = np.einsum("bnk,bk->bn", H, xl) - c
    assert float(np.abs(gx).max()) <= 1e-8
    x_star = np.linalg.solve(H.astype(np.float64), c.astype(np.float64)[:, :, None])[:, :, 0].astype(ld)
    for _ in range(3):   # iterative refinement with the residual in extended precision
        r = c - np.einsum("bnk,bk->bn", H, x_star)
        x_star = x_star + np.linalg.solve(H.astype(np.float64), r.astype(np.float64)[:, :, None])[:, :, 0].astype(ld)
    err = np.sqrt(((xl - x_star) ** 2).sum(axis=1))
    bound = np.sqrt((gx ** 2).sum(axis=1)) / ld(lam) * (ld(1.0) + ld(1e-6))
    assert np.all(err <= bound), float((err - bound).max())


def test_max_rounds_exceeded_raises(gpu_solver_factory):
    import torch
    import cppnumericalsolvers_amd as amd
    solver = gpu_solver_factory(m=6, stopping_progress=_stop(at_lib.base_stop()))
    x0d = torch.from_numpy(at_lib.starts("rosenbrock", 9, 8, seed=1)).to(solver.device)
    with pytest.raises(RuntimeError, match="still active after max_rounds = 3"):
        solver.minimize_callable(lambda X: solver.evaluate(amd.Rosenbrock(), X), x0d, max_rounds=3)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_launch_nothing():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    ctx = amd.Context(0)
    try:
        lib = ctx._lib
        x0 = torch.zeros(4, 8, dtype=torch.float64, device="cuda:0")
        keep = []

        def desc(**over):
            d = capi.Desc()
            d.objective, d.linesearch, d.n, d.m = capi.OBJ_ROSENBROCK, capi.LS_MORE_THUENTE, 8, 6
            d.stop = capi.default_stop()
            for k, v in over.items():
                setattr(d, k, v)
            return d

        diag = np.ones(8)
        keep.append(diag)
        trace = amd.Trace([0], 4, 8, "cuda:0")
        cases = [
            (desc(linesearch=capi.LS_HAGER_ZHANG), capi.ERR_UNSUPPORTED, "Hager-Zhang"),
            (desc(arithmetic=capi.ARITH_FMA), capi.ERR_UNSUPPORTED, "MI355_ARITH_FMA"),
            (desc(history_placement=capi.HISTORY_Y_IN_REGISTERS), capi.ERR_UNSUPPORTED, "MI355_HISTORY_Y_IN_REGISTERS"),
            (desc(hessian_from_functor=1), capi.ERR_UNSUPPORTED, "hessian_from_functor"),
            (desc(hessian_diagonal=diag.ctypes.data_as(C.POINTER(C.c_double))), capi.ERR_UNSUPPORTED, "hessian_diagonal"),
            (desc(hessian_condition_stop=10.0), capi.ERR_UNSUPPORTED, "hessian_condition_stop"),
            (desc(trace=trace.c_pointer()), capi.ERR_UNSUPPORTED, "trace"),
            (desc(per_problem_data=x0.data_ptr(), per_problem_stride=8), capi.ERR_UNSUPPORTED, "per_problem_data"),
            (desc(n=257), capi.ERR_UNSUPPORTED, "n <= 256"),
            (desc(lanes_per_problem=16, elems_per_lane=2), capi.ERR_UNSUPPORTED, "mapping"),
            (desc(lanes_per_problem=4, elems_per_lane=2), capi.ERR_UNSUPPORTED, "mapping"),
            # validate()'s argument errors stay argument errors
            (desc(m=0), capi.ERR_INVALID_ARGUMENT, "m out of range"),
            (desc(n=0), capi.ERR_INVALID_ARGUMENT, "n out of range"),
            (desc(arithmetic=7), capi.ERR_INVALID_ARGUMENT, "arithmetic"),
        ]
        for d, code, text in cases:
            h = C.c_void_p()
            rc = lib.mi355_lbfgs_ask_tell_create(ctx.handle, C.byref(d), 4, x0.data_ptr(), None, C.byref(h))
            message = lib.mi355_lbfgs_last_error().decode()
            assert rc == code and text in message and not h.value, (text, rc, message)
        # the objective and its parameter fields are not read: an id no library knows is accepted
        d = desc(objective=4242, n_params=3)
        h = C.c_void_p()
        capi.check(lib.mi355_lbfgs_ask_tell_create(ctx.handle, C.byref(d), 4, x0.data_ptr(), None, C.byref(h)))
        capi.check(lib.mi355_lbfgs_ask_tell_destroy(h))
        v = [C.c_int32(-1) for _ in range(6)]
        capi.check(lib.mi355_lbfgs_last_launch(ctx.handle, *[C.byref(t) for t in v]))
        assert [t.value for t in v] == [0] * 6, "a refused (or merely created) solve launched a solve kernel"
    finally:
        ctx.close()


def test_solver_configured_with_a_refused_option_raises_the_librarys_message():
    import torch
    import cppnumericalsolvers_amd as amd
    ctx = amd.Context(0)
    try:
        x0 = torch.zeros(4, 8, dtype=torch.float64, device="cuda:0")
        for kw, text in ((dict(linesearch="hager_zhang"), "Hager-Zhang"), (dict(arithmetic="fma"), "MI355_ARITH_FMA"),
                         (dict(history_placement=2), "MI355_HISTORY_Y_IN_REGISTERS"),
                         (dict(condition_hessian=5.0), "hessian_condition_stop")):
            solver = amd.BatchedLbfgs(m=6, context=ctx, **kw)
            with pytest.raises(amd.capi.EngineError) as e:
                solver.minimize_callable(lambda X: (X.sum(dim=1), torch.ones_like(X)), x0)
            assert e.value.code == amd.capi.ERR_UNSUPPORTED and text in str(e.value), str(e.value)
        with pytest.raises(ValueError):
            amd.LbfgsAskTell(amd.BatchedLbfgs(m=6, context=ctx, dtype=torch.float32), x0)
        with pytest.raises(TypeError):
            amd.LbfgsAskTell(amd.BatchedBfgs(context=ctx), x0)
    finally:
        ctx.close()


# ---- 6. the C++ header -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["at_header_test", "at_header_test_noexcept"])
def test_cpp_header_binary_matches_the_persistent_kernel(gpu_solver_factory, binary):
    import torch
    import cppnumericalsolvers_amd as amd
    path = os.path.join(at_lib.TWIN_DIR, "_build", binary)
    assert os.access(path, os.X_OK), "%s is not built (run __graft_entry__.build())" % path
    out = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    n, m, Bc = 13, 6, 5
    x0 = np.array([[(1.0 if j % 2 else -1.2) + 0.0625 * b for j in range(n)] for b in range(Bc)])
    stop = at_lib.base_stop()
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    x, f, g, p = _host(amd, solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to(solver.device)))

    def hexes(a):
        return [format(int(v), "016x") for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]

    lines = out.stdout.splitlines()
    assert sum(line.startswith("rounds ") for line in lines) == 2
    for tag in ("handle", "one_call"):
        rows = [line.split() for line in lines if line.startswith(tag + " ")]
        assert len(rows) == Bc, out.stdout
        for b, w in enumerate(rows):
            want = ([tag, str(b), "status", str(p["status"][b]), "iterations", str(p["num_iterations"][b]), "nfev",
                     str(p["nfev"][b]), "sum_k", str(p["sum_k"][b]), "x_delta"] + hexes(p["x_delta"][b]) + ["f_delta"] +
                    hexes(p["f_delta"][b]) + ["gradient_norm"] + hexes(p["gradient_norm"][b]) + ["f"] + hexes(f[b]) +
                    ["x"] + hexes(x[b]) + ["g"] + hexes(g[b]))
            assert w == want, (tag, b)
    if binary == "at_header_test":
        mis = subprocess.run([path, "--misuse"], capture_output=True, text=True, timeout=120)
        assert mis.returncode == 0 and mis.stdout.startswith("ok: Hager-Zhang"), mis.stdout + mis.stderr
