"""The ask/tell (reverse communication) L-BFGS-B on the device: mi355_lbfgsb_ask_tell_*, amd.LbfgsbAskTell,
BatchedLbfgsb.minimize_callable and the C++ header.

Fed the library's own evaluation entry as the callback, the ask/tell path returns the bits of the persistent
reference-order kernel (BatchedLbfgsb(arithmetic="exact")): x, f, g and every progress field, on every problem — with no
box, a shared box and one box per problem, from infeasible and hostile starts, on degenerate boxes.  The ask counters show
that every cut of the iteration is exercised; an objective written in torch ops reaches its closed-form bounded minimiser;
every refusal names its reason and launches nothing; the C++ header test binary reproduces the persistent kernel too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import at_lib
import atb_lib
import oracle_lib

pytestmark = pytest.mark.gpu
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
B = atb_lib.B


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


def _solver(amd, factory, m=5, stop=None, box=None, rows=None, context=None, **kw):
    """a reference-order BatchedLbfgsb on the session's context with a shared box, rows, or no box"""
    s = amd.BatchedLbfgsb(m=m, stopping_progress=_stop(stop or at_lib.base_stop()), arithmetic="exact",
                          context=context or factory().ctx, **kw)
    if box is not None:
        s.SetBounds(*box)
    if rows is not None:
        s.SetBoundsPerProblem(*rows)
    return s


def _both(amd, solver, objective, x0, evaluator=None, **kw):
    """(persistent kernel, ask/tell with the library's evaluation entry as the callback, rounds) on the same device batch;
    evaluator: the solver whose evaluation entry is the callback (default: `solver` itself)"""
    import torch
    x0d = torch.from_numpy(np.ascontiguousarray(x0)).to(solver.device)
    want = _host(amd, solver.minimize(objective, x0d))
    rounds = [0]

    def fn(X):
        rounds[0] += 1
        return (evaluator or solver).evaluate(objective, X)

    got = _host(amd, solver.minimize_callable(fn, x0d, **kw))
    return got, want, rounds[0]


def _by_hand(amd, solver, objective, x0, max_rounds=100000):
    """the loop over the handle; returns (results, asks, rounds)"""
    import torch
    x0d = torch.from_numpy(np.ascontiguousarray(x0)).to(solver.device)
    with amd.LbfgsbAskTell(solver, x0d) as at:
        active, rounds = at.B, 0
        while active > 0:
            assert rounds < max_rounds, "the batch did not finish"
            active = at.tell(*solver.evaluate(objective, at.x))
            rounds += 1
        return _host(amd, at.results()), at.asks, rounds


# ---- 1. the parity grid --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", atb_lib.HISTORIES)
@pytest.mark.parametrize("n", atb_lib.DIMS)
@pytest.mark.parametrize("objective", ["rosenbrock", "diag_quadratic"])
def test_parity_grid_persistent_kernel_and_oracle(gpu_solver_factory, objective, n, m):
    import cppnumericalsolvers_amd as amd
    stop = at_lib.base_stop()
    lo, hi = atb_lib.box_of(objective, n)
    x0 = at_lib.starts(objective, B, n, seed=2000 * n + m)
    solver = _solver(amd, gpu_solver_factory, m=m, stop=stop, box=(lo, hi))
    got, want, rounds = _both(amd, solver, _objective(amd, objective, n), x0)
    what = "%s n=%d m=%d" % (objective, n, m)
    at_lib.assert_same_results(got, want, "ask/tell vs persistent kernel: " + what)
    assert rounds >= int(want[3]["nfev"].max())
    ll = solver.last_launch()
    assert (ll["lanes_per_problem"], ll["elems_per_lane"]) == (16, atb_lib.width(n) // 16)
    ora = oracle_lib.lbfgsb_minimize_batch(objective, x0, m=m, stop=stop, params=at_lib.params_of(objective, n), lower=lo,
                                           upper=hi, reduction="butterfly", width=atb_lib.width(n))
    at_lib.assert_same_results(got, ora, "ask/tell vs oracle: " + what)


# ---- 2. no box ----------------------------------------------------------------------------------------------------------------
def test_no_box(gpu_solver_factory):
    import cppnumericalsolvers_amd as amd
    x0 = at_lib.starts("rosenbrock", B, 17, seed=17)
    got, want, _ = _both(amd, _solver(amd, gpu_solver_factory, m=5), amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got, want, "no box")


# ---- 3. one box per problem ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [5, 7])
@pytest.mark.parametrize("n", [17, 40])
def test_one_box_per_problem(gpu_solver_factory, n, m):
    import cppnumericalsolvers_amd as amd
    lo, hi = atb_lib.box_of("rosenbrock", n)
    rows = atb_lib.random_rows(lo, hi, seed=300 + n)
    x0 = at_lib.starts("rosenbrock", B, n, seed=30 + n)
    got, want, _ = _both(amd, _solver(amd, gpu_solver_factory, m=m, rows=rows), amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got, want, "one box per problem n=%d m=%d" % (n, m))
    assert np.all(got[0] >= rows[0]) and np.all(got[0] <= rows[1])
    # the same box in every row: the shared-box run
    same_rows = (np.tile(lo, (B, 1)), np.tile(hi, (B, 1)))
    got_rows, _, _ = _both(amd, _solver(amd, gpu_solver_factory, m=m, rows=same_rows), amd.Rosenbrock(), x0)
    got_shared, _, _ = _both(amd, _solver(amd, gpu_solver_factory, m=m, box=(lo, hi)), amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got_rows, got_shared, "equal rows vs the shared box n=%d m=%d" % (n, m))


# ---- 4. infeasible starts -------------------------------------------------------------------------------------------------------
def test_infeasible_starts(gpu_solver_factory):
    import torch
    import cppnumericalsolvers_amd as amd
    n = 33
    x0, outside = atb_lib.infeasible_starts(n, seed=44)
    assert 0 < int(outside.sum()) < B
    solver = _solver(amd, gpu_solver_factory, m=5, box=atb_lib.box_of("rosenbrock", n))
    want = _host(amd, solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to(solver.device)))
    got, asks, _ = _by_hand(amd, solver, amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got, want, "infeasible starts")
    assert asks["clip_start"] == int(outside.sum()), (asks, int(outside.sum()))
    assert asks["first"] == B


# ---- 5. degenerate boxes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", sorted(["pinned", "all_pinned", "crossed", "infinite", "half_infinite", "tiny_box", "huge"]))
def test_degenerate_boxes(gpu_solver_factory, box):
    """the boxes, dimensions and stops of test_gpu_parity.py::test_lbfgsb_degenerate_boxes_match_oracle"""
    import torch
    import cppnumericalsolvers_amd as amd
    for n in (12, 40):
        x0 = np.random.default_rng(5).uniform(-2, 2, (B, n))
        lo, hi = oracle_lib.degenerate_boxes(n)[box]
        for stop in (oracle_lib.lbfgsb_default_stop(), oracle_lib.parity_stop()):
            solver = _solver(amd, gpu_solver_factory, m=5, stop=stop, box=(lo, hi))
            want = _host(amd, solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to(solver.device)))
            got, asks, _ = _by_hand(amd, solver, amd.Rosenbrock(), x0)
            at_lib.assert_same_results(got, want, "%s n=%d" % (box, n))
            assert sum(asks.values()) == int(got[3]["nfev"].sum())
            if box == "all_pinned":
                assert asks["cauchy"] > 0 and asks["trial"] == 0, asks


def test_nan_bound_is_refused(gpu_solver_factory):
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    solver = _solver(amd, gpu_solver_factory, m=5)
    nan_lo, nan_hi = oracle_lib.degenerate_boxes(6)["nan_bound"]
    with pytest.raises(ValueError):
        solver.SetBounds(nan_lo, nan_hi)
    # past the Python check: the C entry refuses as well, for a shared box and for rows
    x0 = torch.zeros(2, 6, dtype=torch.float64, device=solver.device)
    solver._lower = torch.from_numpy(nan_lo).to(solver.device)
    solver._upper = torch.from_numpy(nan_hi).to(solver.device)
    with pytest.raises(capi.EngineError) as e:
        amd.LbfgsbAskTell(solver, x0)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "NaN bound" in str(e.value)
    solver._lower = solver._upper = None
    solver._rows = (torch.from_numpy(np.tile(nan_lo, (2, 1))).to(solver.device),
                    torch.from_numpy(np.tile(nan_hi, (2, 1))).to(solver.device))
    with pytest.raises(capi.EngineError) as e:
        amd.LbfgsbAskTell(solver, x0)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "NaN bound" in str(e.value)


# ---- 6. hostile starts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 20, 40])
def test_hostile_starts(gpu_solver_factory, n):
    """NaN / inf coordinates and overflowing magnitudes under the box [-1.5, 0.8], at the dimensions of
    test_gpu_parity.py::test_non_finite_and_overflowing_starts_match_oracle; NaNs included, bit for bit, sign and payload
    too.  The callback is the library's evaluation entry in the mapping of the L-BFGS-B kernels (16 lanes x E): a NaN
    gradient is handed through as the evaluation made it, and the entry's default mapping of n = 40 (64 lanes x 1) gives
    the NaN of g[4 i + 2] the other sign (measured: 10 entries of the start with x[0] = NaN, all NaN against NaN, none
    at n = 6 and n = 20, none in the 16 x 4 mapping)."""
    import cppnumericalsolvers_amd as amd
    stop = at_lib.base_stop(num_iterations=40)
    x0 = np.concatenate([oracle_lib.hostile_starts(n), at_lib.starts("rosenbrock", B - 10, n, seed=6)])
    solver = _solver(amd, gpu_solver_factory, m=5, stop=stop, box=atb_lib.box_of("rosenbrock", n))
    same_mapping = gpu_solver_factory(lanes_per_problem=16, elems_per_lane=atb_lib.width(n) // 16)
    got, want, _ = _both(amd, solver, amd.Rosenbrock(), x0, evaluator=same_mapping)
    at_lib.assert_same_results(got, want, "hostile starts n=%d" % n)


# ---- 7. every cut of the iteration is exercised ---------------------------------------------------------------------------------
def test_every_cut_is_exercised(gpu_solver_factory):
    import torch
    import cppnumericalsolvers_amd as amd
    x0, lo, hi = atb_lib.every_cut_case()
    solver = _solver(amd, gpu_solver_factory, m=atb_lib.EVERY_CUT["m"], rows=(lo, hi))
    want = _host(amd, solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to(solver.device)))
    got, asks, rounds = _by_hand(amd, solver, amd.Rosenbrock(), x0)
    print("every cut: asks %s in %d rounds" % (asks, rounds))
    at_lib.assert_same_results(got, want, "every cut")
    assert set(asks) == set(atb_lib.ASK_KINDS)
    for kind in atb_lib.ASK_KINDS:
        assert asks[kind] > 0, (kind, asks)
    assert asks["first"] == B
    assert sum(asks.values()) == int(got[3]["nfev"].sum()), (asks, int(got[3]["nfev"].sum()))


# ---- 8. the handle protocol and poisoned rows -----------------------------------------------------------------------------------
def test_handle_protocol_and_poisoned_rows(gpu_solver_factory):
    """LbfgsbAskTell by hand: .x is a view of the library's buffer (no copy), results() at any time, the rows of finished
    problems and of problems in the no-evaluation phase are never read (NaN is handed back for them), extra rounds
    change nothing, close() is idempotent.  Three starts sit on the unconstrained minimiser (g = 0: the search is refused
    at once).  Which rows a round does not read is taken from a clean run first: those whose nfev the round left alone."""
    import torch
    import cppnumericalsolvers_amd as amd
    n = 17
    x0 = at_lib.starts("rosenbrock", B, n, seed=88)
    x0[:3] = 1.0
    solver = _solver(amd, gpu_solver_factory, m=5, box=(np.full(n, -1.5), np.full(n, 1.5)))
    x0d = torch.from_numpy(x0).to(solver.device)
    want = _host(amd, solver.minimize(amd.Rosenbrock(), x0d))
    unread = []   # per round: the rows the step does not read
    with amd.LbfgsbAskTell(solver, x0d) as clean:
        active, before = B, np.zeros(B, dtype=np.int64)
        while active > 0:
            active = clean.tell(*solver.evaluate(amd.Rosenbrock(), clean.x))
            after = _host(amd, clean.results())[3]["nfev"].astype(np.int64)
            unread.append(after == before)
            before = after
            assert len(unread) < 5000
    assert any(np.any(u[:3]) for u in unread[:3]), "no problem went through the no-evaluation phase"
    with amd.LbfgsbAskTell(solver, x0d) as at:
        assert at.x.shape == (B, n) and at.x.dtype == torch.float64 and at.x.data_ptr() != x0d.data_ptr()
        ptr = at.x.data_ptr()
        assert torch.equal(at.x, x0d) and at.active == B
        first = _host(amd, at.results())
        assert np.array_equal(first[0], x0) and np.all(first[3]["status"] == -1)
        for r, mask in enumerate(unread):
            f, g = solver.evaluate(amd.Rosenbrock(), at.x)
            poison = torch.from_numpy(mask).to(solver.device)
            f[poison] = float("nan")
            g[poison] = float("nan")
            active = at.tell(f, g)
            assert active == at.active and at.x.data_ptr() == ptr
        assert active == 0
        for _ in range(3):   # a finished batch stays as it is
            assert at.tell(torch.full_like(f, float("nan")), torch.full_like(g, float("nan"))) == 0
        got = _host(amd, at.results())
        assert np.array_equal(at.x.cpu().numpy(), got[0])   # the evaluation buffer holds the returned x
    at.close()
    at_lib.assert_same_results(got, want, "by hand, NaN rows for finished and no-evaluation problems")
    with pytest.raises(RuntimeError):
        at.tell(f, g)
    with pytest.raises(RuntimeError):
        at.asks


# ---- 9. driver variations ---------------------------------------------------------------------------------------------------------
VARIATION = dict(n=33, m=6, seed=919)


def _variation_inputs():
    v = VARIATION
    return at_lib.starts("rosenbrock", B, v["n"], seed=v["seed"]), atb_lib.box_of("rosenbrock", v["n"])


def test_check_every_7(gpu_solver_factory):
    import cppnumericalsolvers_amd as amd
    x0, box = _variation_inputs()
    solver = _solver(amd, gpu_solver_factory, m=VARIATION["m"], box=box)
    got, want, rounds = _both(amd, solver, amd.Rosenbrock(), x0, check_every=7)
    at_lib.assert_same_results(got, want, "check_every=7")
    assert rounds % 7 == 0
    got1, _, rounds1 = _both(amd, solver, amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got1, want, "check_every=1")
    assert rounds1 <= rounds < rounds1 + 7


def test_non_default_stream(gpu_solver_factory):
    import torch
    import cppnumericalsolvers_amd as amd
    x0, box = _variation_inputs()
    solver = _solver(amd, gpu_solver_factory, m=VARIATION["m"], box=box)
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
    x0, box = _variation_inputs()
    _, want, _ = _both(amd, _solver(amd, gpu_solver_factory, m=VARIATION["m"], box=box), amd.Rosenbrock(), x0)
    monkeypatch.setenv(CAP_ENV, "1")
    ctx = amd.Context(0)
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        solver = _solver(amd, gpu_solver_factory, m=VARIATION["m"], box=box, context=ctx)
        got, asks, _ = _by_hand(amd, solver, amd.Rosenbrock(), x0)
        assert solver.last_launch()["blocks"] == 1
    finally:
        ctx.close()
    at_lib.assert_same_results(got, want, "one workgroup")
    assert sum(asks.values()) == int(got[3]["nfev"].sum())


def test_max_rounds_exceeded_raises(gpu_solver_factory):
    import torch
    import cppnumericalsolvers_amd as amd
    solver = _solver(amd, gpu_solver_factory, m=5, box=atb_lib.box_of("rosenbrock", 8))
    x0d = torch.from_numpy(at_lib.starts("rosenbrock", 9, 8, seed=1)).to(solver.device)
    with pytest.raises(RuntimeError, match="still active after max_rounds = 3"):
        solver.minimize_callable(lambda X: solver.evaluate(amd.Rosenbrock(), X), x0d, max_rounds=3)


# ---- 10. an objective the library does not have -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["value_and_gradient", "value_only"])
@pytest.mark.parametrize("n", atb_lib.TORCH_DIMS)
def test_objective_written_in_torch_ops(gpu_solver_factory, n, form):
    """f_b(x) = sum a_i (x_i - c_{b,i})^2 in torch ops under one box per problem: the minimiser is clip(c_b, lo_b, hi_b).
    The stop test reads the projected gradient of the iterate the last step started from, so the bound is not a theorem:
    the draw is the one tests/test_ask_tell_box_cpu.py clears on the CPU oracle (2.46e-9 at n = 13, 4.62e-9 at n = 40).
    Prints the measured maximum (MI355X: 2.46e-9 at n = 13, 4.59e-9 at n = 40, the same for both forms)."""
    import torch
    import cppnumericalsolvers_amd as amd
    a, c, lo, hi, x0 = atb_lib.torch_case(n)
    solver = _solver(amd, gpu_solver_factory, m=atb_lib.TORCH_M, stop=atb_lib.torch_case_stop(), rows=(lo, hi))
    ad, cd = torch.from_numpy(a).to(solver.device), torch.from_numpy(c).to(solver.device)

    def value(X):
        r = X - cd
        return (ad * r * r).sum(dim=1)

    def value_and_gradient(X):
        r = X - cd
        return (ad * r * r).sum(dim=1), 2.0 * ad * r

    fn = value if form == "value_only" else value_and_gradient
    x, f, g, p = _host(amd, solver.minimize_callable(fn, torch.from_numpy(x0).to(solver.device), max_rounds=5000))
    err = float(np.max(np.abs(x - np.clip(c, lo, hi))))
    print("torch-op bounded quadratic n=%d %s: max|x - clip(c)| = %.3g" % (n, form, err))
    assert np.all(x >= lo) and np.all(x <= hi)
    assert np.all(p["status"] == atb_lib.GRADIENT_STATUS), np.unique(p["status"], return_counts=True)
    assert err <= at_lib.CONTRACT


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_launch_nothing():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    ctx = amd.Context(0)
    try:
        lib = ctx._lib
        x0 = torch.zeros(4, 8, dtype=torch.float64, device="cuda:0")

        def desc(**over):
            d = capi.Desc()
            d.objective, d.linesearch, d.n, d.m = capi.OBJ_ROSENBROCK, capi.LS_MORE_THUENTE, 8, 5
            d.stop = capi.default_stop("lbfgsb")
            for k, v in over.items():
                setattr(d, k, v)
            return d

        def create(d, lower=None, upper=None, stride=0):
            h = C.c_void_p()
            rc = lib.mi355_lbfgsb_ask_tell_create(ctx.handle, C.byref(d), lower, upper, stride, 4, x0.data_ptr(), None,
                                                  C.byref(h))
            return rc, lib.mi355_lbfgs_last_error().decode(), h

        diag = np.ones(8)
        trace = amd.Trace([0], 4, 8, "cuda:0")
        cases = [
            (desc(linesearch=capi.LS_HAGER_ZHANG), "Hager-Zhang"),
            (desc(arithmetic=capi.ARITH_FMA), "MI355_ARITH_FMA"),
            (desc(m=9), "m <= 8"),
            (desc(m=10), "m <= 8"),
            (desc(n=65), "n <= 64"),
            (desc(trace=trace.c_pointer()), "trace"),
            (desc(per_problem_data=x0.data_ptr(), per_problem_stride=8), "per_problem_data"),
            (desc(hessian_from_functor=1), "hessian_from_functor"),
            (desc(hessian_diagonal=diag.ctypes.data_as(C.POINTER(C.c_double))), "hessian_diagonal"),
            (desc(hessian_condition_stop=10.0), "hessian_condition_stop"),
            (desc(lanes_per_problem=16), "lanes_per_problem"),
            (desc(elems_per_lane=1), "elems_per_lane"),
            (desc(history_placement=capi.HISTORY_Y_IN_REGISTERS), "history_placement"),
        ]
        for d, text in cases:
            rc, message, h = create(d)
            assert rc == capi.ERR_UNSUPPORTED and message.startswith("Lbfgsb ask/tell") and text in message \
                and not h.value, (text, rc, message)
        # argument errors stay argument errors
        for d, kw, text in ((desc(m=0), {}, "m out of range"), (desc(n=0), {}, "n out of range"),
                            (desc(), dict(lower=x0.data_ptr()), "both"),
                            (desc(), dict(lower=x0.data_ptr(), upper=x0.data_ptr(), stride=7), "box_stride")):
            rc, message, h = create(d, **kw)
            assert rc == capi.ERR_INVALID_ARGUMENT and text in message and not h.value, (text, rc, message)
        # the objective and its parameter fields are not read; MI355_ARITH_DEFAULT is the exact arithmetic here
        rc, message, h = create(desc(objective=4242, n_params=3, arithmetic=capi.ARITH_DEFAULT))
        assert rc == 0, message
        capi.check(lib.mi355_lbfgsb_ask_tell_destroy(h))
        v = [C.c_int32(-1) for _ in range(6)]
        capi.check(lib.mi355_lbfgs_last_launch(ctx.handle, *[C.byref(t) for t in v]))
        assert [t.value for t in v] == [0] * 6, "a refused (or merely created) solve launched a solve kernel"
    finally:
        ctx.close()


def test_python_refusals():
    import torch
    import cppnumericalsolvers_amd as amd
    ctx = amd.Context(0)
    try:
        x0 = torch.zeros(4, 8, dtype=torch.float64, device="cuda:0")

        def fn(X):
            return X.sum(dim=1), torch.ones_like(X)

        for kw, text in ((dict(linesearch="hager_zhang"), "Hager-Zhang"), (dict(arithmetic="fma"), "MI355_ARITH_FMA"),
                         (dict(m=9), "m <= 8")):
            with pytest.raises(amd.capi.EngineError) as e:
                amd.BatchedLbfgsb(context=ctx, **kw).minimize_callable(fn, x0)
            assert e.value.code == amd.capi.ERR_UNSUPPORTED and text in str(e.value), str(e.value)
        with pytest.raises(amd.capi.EngineError) as e:
            amd.BatchedLbfgsb(context=ctx).minimize_callable(fn, torch.zeros(4, 65, dtype=torch.float64, device="cuda:0"))
        assert "n <= 64" in str(e.value)
        with pytest.raises(ValueError):   # float: the solver class is float64 only
            amd.BatchedLbfgsb(context=ctx, dtype=torch.float32)
        with pytest.raises(TypeError):
            amd.LbfgsbAskTell(amd.BatchedLbfgs(m=5, context=ctx), x0)
        with pytest.raises(TypeError):
            amd.LbfgsAskTell(amd.BatchedLbfgsb(m=5, context=ctx), x0)
        with pytest.raises(TypeError):
            amd.BatchedBfgs(context=ctx).minimize_callable(fn, x0)
        rows = amd.BatchedLbfgsb(context=ctx)
        rows.SetBoundsPerProblem(np.zeros((3, 8)), np.ones((3, 8)))
        with pytest.raises(ValueError, match="per-problem bounds are"):   # the [B, n] check of the rows
            rows.minimize_callable(fn, x0)
    finally:
        ctx.close()


# ---- 12. the C++ header ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["atb_header_test", "atb_header_test_noexcept"])
def test_cpp_header_binary_matches_the_persistent_kernel(gpu_solver_factory, binary):
    import torch
    import cppnumericalsolvers_amd as amd
    path = os.path.join(atb_lib.BOX_DIR, "_build", binary)
    assert os.access(path, os.X_OK), "%s is not built (run __graft_entry__.build())" % path
    out = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    n, m, Bc = 13, 5, 5
    x0 = np.array([[(1.0 if j % 2 else -1.2) + 0.0625 * b + (1.0 if b >= 3 else 0.0) for j in range(n)] for b in range(Bc)])
    lo_rows = np.array([[-1.5 - b / 32.0] * n for b in range(Bc)])
    hi_rows = np.array([[0.8 + b / 16.0] * n for b in range(Bc)])
    boxes = dict(none={}, shared=dict(box=(np.full(n, -1.5), np.full(n, 0.8))), rows=dict(rows=(lo_rows, hi_rows)))

    def hexes(a):
        return [format(int(v), "016x") for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]

    lines = out.stdout.splitlines()
    for tag, kw in boxes.items():
        solver = _solver(amd, gpu_solver_factory, m=m, **kw)
        x, f, g, p = _host(amd, solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to(solver.device)))
        rows = [line.split() for line in lines if line.startswith(tag + " ")]
        assert len(rows) == Bc, out.stdout
        for b, w in enumerate(rows):
            want = ([tag, str(b), "status", str(p["status"][b]), "iterations", str(p["num_iterations"][b]), "nfev",
                     str(p["nfev"][b]), "sum_k", str(p["sum_k"][b]), "x_delta"] + hexes(p["x_delta"][b]) + ["f_delta"] +
                    hexes(p["f_delta"][b]) + ["gradient_norm"] + hexes(p["gradient_norm"][b]) + ["f"] + hexes(f[b]) +
                    ["x"] + hexes(x[b]) + ["g"] + hexes(g[b]))
            assert w == want, (tag, b)
        summary = [line.split() for line in lines if line.startswith("rounds %s " % tag)]
        assert len(summary) == 1
        asks = [int(v) for v in summary[0][4:9]]
        assert sum(asks) == int(p["nfev"].sum()) and asks[4] == Bc
        assert (asks[0] > 0) == (tag != "none")   # two starts lie outside every box there is
    if binary == "atb_header_test":
        mis = subprocess.run([path, "--misuse"], capture_output=True, text=True, timeout=120)
        assert mis.returncode == 0 and mis.stdout.startswith("ok: Hager-Zhang"), mis.stdout + mis.stderr
