"""The ask/tell (reverse communication) L-BFGS ABOVE n = 256 on the device: mi355_lbfgs_ask_tell_wide_*, picked by
amd.LbfgsAskTell / BatchedLbfgs.minimize_callable for a float64 solver when x0 has more than 256 columns; and
mi355_lbfgs_eval_batch (BatchedLbfgs.evaluate) above n = 256.

The reference of the bit-for-bit comparisons is the oracle's Lbfgs::Minimize in the strided order of the kernel's T
threads (oracle.minimize_batch(reduction="strided", width=T), T = 256, 1024 from n = 32768 on) and, for single
evaluations and the round-by-round run, the oracle's functors in that same order (atw_lib.evaluate, the stepper of
tests/ask_tell_wide/atw_twin.hpp).  oracle_lib.evaluate(reduction="strided") is not used: it does not know the order
(atw_lib.evaluate's docstring)."""
import ctypes as C

import numpy as np
import pytest

import at_lib
import atw_lib
import oracle_lib

pytestmark = pytest.mark.gpu
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
LDS_ENV = "MI355_WIDE_LDS_MAX_N"


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


def _ask_tell(amd, solver, objective, x0, **kw):
    """minimize_callable with the library's evaluation entry as the callback; returns (results, rounds)"""
    import torch
    rounds = [0]

    def fn(X, *ids):
        rounds[0] += 1
        return solver.evaluate(objective, X)

    return _host(amd, solver.minimize_callable(fn, torch.from_numpy(x0).to(solver.device), **kw)), rounds[0]


def _persistent(amd, solver, objective, x0):
    import torch
    return _host(amd, solver.minimize(objective, torch.from_numpy(x0).to(solver.device)))


# ---- 1. the anchor: ask/tell == the persistent wide kernel == the strided oracle ------------------------------------------
ANCHOR = [(o, n, m, B, s, None) for (o, n, m, B) in (("rosenbrock", 257, 6, 9), ("rosenbrock", 300, 10, 40),
                                                       ("diag_quadratic", 513, 17, 8))
          for s in ("default", "parity", "conservative")] + [
    ("rosenbrock", 1000, 5, 12, "parity", 400),
    ("diag_quadratic", 4097, 6, 3, "parity", None),     # just past the direction-in-LDS form
    ("diag_quadratic", 5000, 32, 3, "parity", None),    # m at its cap
    ("diag_quadratic", 32768, 4, 2, "parity", 30),      # 1024 threads per problem
]


@pytest.mark.parametrize("objective,n,m,B,stop_name,limit", ANCHOR)
def test_callback_of_the_librarys_own_evaluation_is_the_persistent_kernel_and_the_oracle(gpu_solver_factory, objective, n,
                                                                                         m, B, stop_name, limit):
    import cppnumericalsolvers_amd as amd
    stop = atw_lib.stops()[stop_name]
    if limit is not None:
        stop.num_iterations = limit
    x0 = at_lib.starts(objective, B, n, seed=1000 + n + m)
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    obj = _objective(amd, objective, n)
    want = _persistent(amd, solver, obj, x0)
    got, rounds = _ask_tell(amd, solver, obj, x0)
    launch = solver.last_launch()
    what = "%s n=%d m=%d %s" % (objective, n, m, stop_name)
    at_lib.assert_same_results(got, want, "ask/tell vs persistent kernel: " + what)
    assert rounds >= int(want[3]["nfev"].max())
    assert launch["threads"] == atw_lib.threads(n), launch
    assert (launch["lds_bytes"] > 0) == (n <= 4096), launch
    oracle = atw_lib.oracle_minimize(objective, x0, m, stop, params=at_lib.params_of(objective, n))
    at_lib.assert_same_results(got, oracle, "ask/tell vs strided oracle: " + what)


# ---- 2. round by round ---------------------------------------------------------------------------------------------------------
def test_every_round_equals_the_twin(gpu_solver_factory):
    """the first 40 rounds of Rosenbrock-300, m = 10, 12 problems: the evaluation buffer after every tell and the active
    count are the twin's; both sides evaluate their own buffer (equal bits in, equal bits out)"""
    import torch
    import cppnumericalsolvers_amd as amd
    n, m, B = 300, 10, 12
    stop = at_lib.base_stop(num_iterations=12)   # (some problems finish inside the 40 rounds)
    x0 = at_lib.starts("rosenbrock", B, n, seed=77)
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    twin = atw_lib.Twin(x0, m, stop)
    try:
        with amd.LbfgsAskTell(solver, torch.from_numpy(x0).to(solver.device)) as at:
            assert at.x.shape == (B, n) and at.active == B
            assert np.array_equal(at.x.cpu().numpy(), x0)
            for r in range(40):
                f, g = solver.evaluate(amd.Rosenbrock(), at.x)
                ft, gt = atw_lib.evaluate("rosenbrock", twin.x.copy())
                assert at_lib.same_bits(f.cpu().numpy(), ft).all() and at_lib.same_bits(g.cpu().numpy(), gt).all(), r
                active = at.tell(f, g)
                assert active == twin.tell(ft, gt), r
                same = at_lib.same_bits(at.x.cpu().numpy(), twin.x)
                assert same.all(), (r, np.nonzero(~same.all(axis=1))[0][:8])
            at_lib.assert_same_results(_host(amd, at.results()), twin.results(), "after 40 rounds")
    finally:
        twin.close()


# ---- 3. a capped grid ----------------------------------------------------------------------------------------------------------
def test_capped_grid_of_three_workgroups_and_tiny_batches(monkeypatch, gpu_solver_factory):
    """37 problems at n = 260 through three workgroups, each striding over a dozen rows: the bits of the uncapped run
    (gpu_solver_factory is asked for first, so that the session's shared context is never created under the cap).
    Then B = 1 and B = 0."""
    import torch
    import cppnumericalsolvers_amd as amd
    n, m, B = 260, 6, 37
    stop = at_lib.base_stop(num_iterations=25)
    x0 = at_lib.starts("rosenbrock", B, n, seed=5)
    free_solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    want, _ = _ask_tell(amd, free_solver, amd.Rosenbrock(), x0)
    assert free_solver.last_launch()["blocks"] == B
    monkeypatch.setenv(CAP_ENV, "3")
    ctx = amd.Context(0)
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        solver = amd.BatchedLbfgs(m=m, stopping_progress=_stop(stop), arithmetic="exact", context=ctx)
        got, _ = _ask_tell(amd, solver, amd.Rosenbrock(), x0)
        assert solver.last_launch()["blocks"] == 3
        listed, _ = _ask_tell(amd, solver, amd.Rosenbrock(), x0, compact_every=2)
    finally:
        ctx.close()
    at_lib.assert_same_results(got, want, "three workgroups")
    at_lib.assert_same_results(listed, want, "three workgroups, listed")
    at_lib.assert_same_results(want, atw_lib.oracle_minimize("rosenbrock", x0, m, stop), "oracle")
    one, _ = _ask_tell(amd, free_solver, amd.Rosenbrock(), x0[:1])
    at_lib.assert_same_results(one, tuple(a[:1] for a in want), "B = 1")
    x, f, g, p = free_solver.minimize_callable(lambda X: free_solver.evaluate(amd.Rosenbrock(), X),
                                               torch.zeros(0, n, dtype=torch.float64, device=free_solver.device))
    assert x.shape == (0, n) and f.shape == (0,) and g.shape == (0, n)
    with amd.LbfgsAskTell(free_solver, torch.zeros(0, n, dtype=torch.float64, device=free_solver.device)) as at:
        assert at.active == 0 and at.compact() == 0


# ---- 4. the edge starts of tests/test_gpu_wide.py ---------------------------------------------------------------------------
def test_hostile_starts_equal_the_strided_oracle(gpu_solver_factory):
    """n = 400: rows with a NaN, +inf and -inf coordinate, the minimiser itself (the search is refused at once: the
    no-evaluation phase), 1e200 and its kin"""
    import cppnumericalsolvers_amd as amd
    n, m = 400, 6
    stop = at_lib.base_stop(num_iterations=40)
    x0 = np.concatenate([oracle_lib.hostile_starts(n), np.ones((2, n)), at_lib.starts("rosenbrock", 2, n, seed=3)])
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    got, _ = _ask_tell(amd, solver, amd.Rosenbrock(), x0)
    at_lib.assert_same_results(got, atw_lib.oracle_minimize("rosenbrock", x0, m, stop), "hostile starts", nan_equal=True)
    at_lib.assert_same_results(got, _persistent(amd, solver, amd.Rosenbrock(), x0), "hostile starts vs persistent",
                               nan_equal=True)
    assert got[3]["nfev"][10] == 1 and got[3]["num_iterations"][10] >= 1   # at the minimiser nothing more was evaluated


# ---- 5. rows of finished problems ------------------------------------------------------------------------------------------------
def test_rows_of_finished_problems_are_never_read(gpu_solver_factory):
    import torch
    import cppnumericalsolvers_amd as amd
    objective, n, m, B = "diag_quadratic", 513, 17, 8
    stop = atw_lib.stops()["parity"]
    x0 = at_lib.starts(objective, B, n, seed=500 + n)
    x0[::2] *= 1e-3   # (every other problem starts close: the batch finishes over several rounds)
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    obj = _objective(amd, objective, n)
    want = _persistent(amd, solver, obj, x0)
    assert len(set(want[3]["nfev"].tolist())) > 1
    poisoned = 0
    with amd.LbfgsAskTell(solver, torch.from_numpy(x0).to(solver.device)) as at:
        active, rounds = B, 0
        while active > 0:
            f, g = solver.evaluate(obj, at.x)
            done = torch.from_numpy(_host(amd, at.results())[3]["status"] > 0).to(solver.device)
            poisoned += int(done.sum())
            f[done] = float("nan")
            g[done] = float("nan")
            active = at.tell(f, g)
            rounds += 1
            assert rounds < 2000
        for _ in range(2):   # a finished batch stays as it is
            assert at.tell(torch.full_like(f, float("nan")), torch.full_like(g, float("nan"))) == 0
        got = _host(amd, at.results())
        assert np.array_equal(at.x.cpu().numpy(), got[0])   # the evaluation buffer holds the returned x
    assert poisoned > 0
    at_lib.assert_same_results(got, want, "NaN rows for finished problems")


# ---- 6. the two homes of the direction ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [500, 2000])
def test_direction_in_lds_and_in_memory_agree(monkeypatch, gpu_solver_factory, n):
    import cppnumericalsolvers_amd as amd
    m, B = 7, 5
    stop = at_lib.base_stop(num_iterations=30)
    x0 = at_lib.starts("rosenbrock", B, n, seed=n)
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    in_lds, _ = _ask_tell(amd, solver, amd.Rosenbrock(), x0)
    assert solver.last_launch()["lds_bytes"] == 8 * (n + n % 2)
    monkeypatch.setenv(LDS_ENV, "0")
    in_memory, _ = _ask_tell(amd, solver, amd.Rosenbrock(), x0)
    assert solver.last_launch()["lds_bytes"] == 0
    monkeypatch.delenv(LDS_ENV, raising=False)
    at_lib.assert_same_results(in_memory, in_lds, "direction in memory vs in LDS")
    at_lib.assert_same_results(in_lds, atw_lib.oracle_minimize("rosenbrock", x0, m, stop), "oracle")


# ---- 7. listed mode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact_every", [1, 3])
def test_listed_mode_equals_the_unlisted_loop(gpu_solver_factory, compact_every):
    """B = 41, n = 300: the loop of minimize_callable(compact_every=k) by hand.  Every list is ascending and holds no
    problem whose status was final at the compaction that made it; the loop ends on an empty list; the results are the
    unlisted loop's bit for bit."""
    import torch
    import cppnumericalsolvers_amd as amd
    objective, n, m, B = "diag_quadratic", 300, 6, 41
    stop = atw_lib.stops()["parity"]
    x0 = at_lib.starts(objective, B, n, seed=41)
    x0[::3] *= 1e-3   # (the batch finishes over several rounds)
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(stop))
    obj = _objective(amd, objective, n)
    want, rounds_unlisted = _ask_tell(amd, solver, obj, x0)
    shorter = 0
    with amd.LbfgsAskTell(solver, torch.from_numpy(x0).to(solver.device)) as at:
        rounds = 0
        while True:
            final = _host(amd, at.results())[3]["status"] > 0
            listed = at.compact()
            if listed == 0:
                break
            ids = at.ids.cpu().numpy()
            assert ids.shape == (listed,) and np.all(np.diff(ids) > 0) and ids.min() >= 0 and ids.max() < B
            assert np.array_equal(ids, np.nonzero(~final)[0])
            assert at.x.shape == (listed, n)
            shorter += int(listed < B)
            for _ in range(compact_every):
                f, g = solver.evaluate(obj, at.x)
                assert f.shape == (listed,)
                rounds += 1
                if at.tell(f, g) == 0:
                    break
            assert rounds < 5000
        assert at.ids.numel() == 0 and at.active == 0
        got = _host(amd, at.results())
    assert shorter > 0 and rounds == rounds_unlisted
    at_lib.assert_same_results(got, want, "listed, compact_every=%d" % compact_every)
    through_loop, _ = _ask_tell(amd, solver, obj, x0, compact_every=compact_every)
    at_lib.assert_same_results(through_loop, want, "minimize_callable(compact_every=%d)" % compact_every)


# ---- 8. a torch objective, values only ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", atw_lib.TORCH_DIMS)
def test_value_only_torch_objective_reaches_the_minimiser(gpu_solver_factory, n):
    """fn(X) = (a * X * X).sum(1) + c with a in [0.5, 20], the gradient by autograd, the gradient test alone
    (1e-8 relative).  At the stop |2 a_j x_j| < 1e-8 max(1, max |x|) with a_j >= 0.5; max |x| < 1 then, so |x_j| < 1e-8
    for every j: the bound is derived, not measured.  (tests/test_ask_tell_wide_twin.py clears the inputs on the CPU.)"""
    import torch
    import cppnumericalsolvers_amd as amd
    a, x0 = atw_lib.torch_case(n)
    assert a.min() >= 0.5 and a.max() <= 20.0
    solver = gpu_solver_factory(m=10, stopping_progress=_stop(atw_lib.torch_case_stop()))
    ad = torch.from_numpy(a).to(solver.device)
    calls = [0]

    def fn(X):
        calls[0] += 1
        return (ad * X * X).sum(1) + atw_lib.TORCH_C

    x, f, g, p = _host(amd, solver.minimize_callable(fn, torch.from_numpy(x0).to(solver.device), max_rounds=3000))
    assert calls[0] > 1
    assert np.all(p["status"] == atw_lib.GRADIENT_STATUS), np.unique(p["status"], return_counts=True)
    assert float(np.abs(x).max()) <= 1e-8
    assert np.all(np.abs(2.0 * a * x) < 1e-8)


# ---- 9. evaluate above n = 256 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 300, 4097, 32768])
@pytest.mark.parametrize("objective", ["rosenbrock", "diag_quadratic"])
def test_evaluate_equals_the_oracles_functor_in_strided_order(gpu_solver_factory, objective, n):
    import torch
    import cppnumericalsolvers_amd as amd
    x = at_lib.starts(objective, 3, n, seed=n)
    solver = gpu_solver_factory(m=6)
    f, g = solver.evaluate(_objective(amd, objective, n), torch.from_numpy(x).to(solver.device))
    torch.cuda.synchronize()
    assert solver.last_launch()["threads"] == atw_lib.threads(n)
    fo, go = atw_lib.evaluate(objective, x, params=at_lib.params_of(objective, n))
    assert at_lib.same_bits(f.cpu().numpy(), fo).all(), (f.cpu().numpy(), fo)
    assert at_lib.same_bits(g.cpu().numpy(), go).all()


def test_evaluate_refuses_other_objectives_above_256(gpu_solver_factory):
    import torch
    import cppnumericalsolvers_amd as amd
    solver = gpu_solver_factory(m=6)
    n = 300
    A = np.ones((4, n))
    with pytest.raises(amd.capi.EngineError) as e:
        solver.evaluate(amd.SquaredErrorRidge(A, 0.1), torch.zeros(2, n, dtype=torch.float64, device=solver.device),
                        per_problem=torch.zeros(2, 4, dtype=torch.float64, device=solver.device))
    assert e.value.code == amd.capi.ERR_UNSUPPORTED and "Rosenbrock and DiagQuadratic" in str(e.value), str(e.value)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_wide_create_name_their_reason_and_launch_nothing():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    ctx = amd.Context(0)
    try:
        lib = ctx._lib
        n = 300
        x0 = torch.zeros(4, n, dtype=torch.float64, device="cuda:0")

        def desc(**over):
            d = capi.Desc()
            d.objective, d.linesearch, d.n, d.m = capi.OBJ_ROSENBROCK, capi.LS_MORE_THUENTE, n, 6
            d.stop = capi.default_stop()
            for k, v in over.items():
                setattr(d, k, v)
            return d

        diag = np.ones(n)
        trace = amd.Trace([0], 4, 8, "cuda:0")
        cases = [
            (desc(n=256), capi.ERR_UNSUPPORTED, "mi355_lbfgs_ask_tell_create"),
            (desc(n=8), capi.ERR_UNSUPPORTED, "mi355_lbfgs_ask_tell_create"),
            (desc(linesearch=capi.LS_HAGER_ZHANG), capi.ERR_UNSUPPORTED, "Hager-Zhang"),
            (desc(arithmetic=capi.ARITH_FMA), capi.ERR_UNSUPPORTED, "MI355_ARITH_FMA"),
            (desc(history_placement=capi.HISTORY_Y_IN_REGISTERS), capi.ERR_UNSUPPORTED, "MI355_HISTORY_Y_IN_REGISTERS"),
            (desc(hessian_from_functor=1), capi.ERR_UNSUPPORTED, "hessian_from_functor"),
            (desc(hessian_diagonal=diag.ctypes.data_as(C.POINTER(C.c_double))), capi.ERR_UNSUPPORTED, "hessian_diagonal"),
            (desc(hessian_condition_stop=10.0), capi.ERR_UNSUPPORTED, "hessian_condition_stop"),
            (desc(trace=trace.c_pointer()), capi.ERR_UNSUPPORTED, "trace"),
            (desc(per_problem_data=x0.data_ptr(), per_problem_stride=8), capi.ERR_UNSUPPORTED, "per_problem_data"),
            (desc(lanes_per_problem=64, elems_per_lane=4), capi.ERR_UNSUPPORTED, "mapping"),
            (desc(lanes_per_problem=64), capi.ERR_UNSUPPORTED, "mapping"),
            (desc(elems_per_lane=2), capi.ERR_UNSUPPORTED, "mapping"),
        ]
        for d, code, text in cases:
            h = C.c_void_p()
            rc = lib.mi355_lbfgs_ask_tell_wide_create(ctx.handle, C.byref(d), 4, x0.data_ptr(), None, C.byref(h))
            message = lib.mi355_lbfgs_last_error().decode()
            assert rc == code and text in message and not h.value, (text, rc, message)
            assert message.startswith("Lbfgs ask/tell wide"), message
        # validate()'s argument errors stay argument errors
        for d, text in ((desc(m=0), "m out of range"), (desc(m=33), "m out of range"), (desc(arithmetic=7), "arithmetic")):
            h = C.c_void_p()
            rc = lib.mi355_lbfgs_ask_tell_wide_create(ctx.handle, C.byref(d), 4, x0.data_ptr(), None, C.byref(h))
            message = lib.mi355_lbfgs_last_error().decode()
            assert rc == capi.ERR_INVALID_ARGUMENT and text in message and not h.value, (text, rc, message)
        # the create for n <= 256 keeps its refusal of this n, in its own words
        h = C.c_void_p()
        d = desc()
        rc = lib.mi355_lbfgs_ask_tell_create(ctx.handle, C.byref(d), 4, x0.data_ptr(), None, C.byref(h))
        assert rc == capi.ERR_UNSUPPORTED and "Lbfgs ask/tell is built for n <= 256" in lib.mi355_lbfgs_last_error().decode()
        # a handle that is only created and destroyed launches no solve kernel either
        capi.check(lib.mi355_lbfgs_ask_tell_wide_create(ctx.handle, C.byref(d), 4, x0.data_ptr(), None, C.byref(h)))
        capi.check(lib.mi355_lbfgs_ask_tell_wide_destroy(h))
        v = [C.c_int32(-1) for _ in range(6)]
        capi.check(lib.mi355_lbfgs_last_launch(ctx.handle, *[C.byref(t) for t in v]))
        assert [t.value for t in v] == [0] * 6, "a refused (or merely created) solve launched a solve kernel"
    finally:
        ctx.close()


def test_float32_solver_above_256_keeps_its_refusal():
    import torch
    import cppnumericalsolvers_amd as amd
    ctx = amd.Context(0)
    try:
        solver = amd.BatchedLbfgs(m=6, context=ctx, dtype=torch.float32)
        x0 = torch.zeros(4, 300, dtype=torch.float32, device="cuda:0")
        with pytest.raises(amd.capi.EngineError) as e:
            solver.minimize_callable(lambda X: (X.sum(dim=1), torch.ones_like(X)), x0)
        assert e.value.code == amd.capi.ERR_UNSUPPORTED and "Lbfgs ask/tell f32 is built for n <= 256" in str(e.value)
        wide = amd.BatchedLbfgs(m=6, context=ctx, lanes_per_problem=64, elems_per_lane=4)
        with pytest.raises(amd.capi.EngineError) as e:
            amd.LbfgsAskTell(wide, torch.zeros(4, 300, dtype=torch.float64, device="cuda:0"))
        assert "Lbfgs ask/tell wide" in str(e.value) and "mapping" in str(e.value)
    finally:
        ctx.close()
