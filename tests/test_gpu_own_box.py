"""One box per problem on the GPU: BatchedLbfgsb.SetBoundsPerProblem, mi355_lbfgsb_minimize_batch_boxes[_host] and
Lbfgsb::MinimizeBatch(function, states, lower, upper).

The inputs (tests/own_box_cases.py): seven cases of 131 problems whose rows cycle through nine boxes, and their twins —
the oracles as they are, called once per box on that box's rows (tests/test_own_box_cpu.py shows that the boxes bind).

4. device == twin, bit for bit (x, f, g, every progress field), under lbfgsb_default_stop and parity_stop, on the
   uncapped grid and on a grid capped to two workgroups (eight segments: sixteen fetches per segment on average, a
   different box at every fetch), capped == uncapped; every x inside its own row's box
5. all rows equal to one box == SetBounds + the shared entry (exact and relaxed, n = 32, m = 5)
6. permuting the problems together with their rows permutes the results
7. host entry == device entry (also through several chunks, and with padded rows); NaN / stride / NULL refusals; what is
   not built is MI355_ERR_UNSUPPORTED and launches nothing; a trace across three boxes
8. the C++ overload == nine single SetBounds + Minimize solves (tests/own_box/own_box_header_test.cc)
9. the exact cases under parity_stop against the reference's own Lbfgsb, each row with its box, within the 1e-6 of
   tests/test_gpu_reference_and_dist.py (m = 7, which the reference binary does not hold on this function: against its
   results as recorded by tests/golden/make_golden_own_box.py)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import own_box_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
CAP = 2
ALL = [c["name"] for c in cases.CASES]


@pytest.fixture
def capped(monkeypatch, gpu_solver_factory):
    """capped(cap, library=None): a fresh context whose resident grid is capped to `cap` workgroups (None: uncapped); the
    variable is read when a context is created (tests/test_gpu_work_queue.py)."""
    import cppnumericalsolvers_amd as amd
    made = []

    def make(cap, library=None):
        if cap is None:
            monkeypatch.delenv(CAP_ENV, raising=False)
        else:
            monkeypatch.setenv(CAP_ENV, str(cap))
        ctx = amd.Context(0, library=library)
        monkeypatch.delenv(CAP_ENV, raising=False)
        made.append(ctx)
        return ctx

    yield make
    for ctx in made:
        ctx.close()


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _engine_stop(oracle_stop):
    from cppnumericalsolvers_amd import capi
    dst = capi.Stop()
    for name, _ in oracle_stop._fields_:
        setattr(dst, name, getattr(oracle_stop, name))
    return dst


def _solver(ctx, oracle, case, preset, arithmetic=None):
    import cppnumericalsolvers_amd as amd
    arithmetic = arithmetic or {"exact": "exact", "relaxed": "fma"}[case["kernel"]]
    return amd.BatchedLbfgsb(m=case["m"], arithmetic=arithmetic, context=ctx,
                             stopping_progress=_engine_stop(cases.stop_of(oracle, preset)))


def _run(solver, case, x0, per_problem=None, trace=None):
    import torch
    import cppnumericalsolvers_amd as amd
    x, f, g, p = solver.minimize(cases.engine_objective(case), _to_dev(x0), trace=trace,
                                 per_problem=None if per_problem is None else _to_dev(per_problem))
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


def _own_box_run(ctx, oracle, name, preset, rows=None, arithmetic=None):
    """The case through SetBoundsPerProblem + minimize on `ctx` (rows: a permutation / subset of the batch)."""
    case = cases.BY_NAME[name]
    x0, lower, upper, pp = cases.inputs(case)
    if rows is not None:
        x0, lower, upper, pp = x0[rows], lower[rows], upper[rows], None if pp is None else pp[rows]
    solver = _solver(ctx, oracle, case, preset, arithmetic)
    solver.SetBoundsPerProblem(lower, upper)
    out = _run(solver, case, x0, pp)
    assert solver.last_arithmetic() == {"exact": "exact", "relaxed": "fma"}[case["kernel"]]
    return out, solver


# ---- 4 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["default", "parity"])
@pytest.mark.parametrize("name", ALL)
def test_device_equals_twin_on_every_grid(capped, gpu_solver_factory, oracle, name, preset):
    case = cases.BY_NAME[name]
    twin = cases.twin(oracle, name, preset)
    _, lower, upper, _ = cases.inputs(case)
    runs = {}
    for cap in (None, CAP):
        ctx = gpu_solver_factory().ctx if cap is None else capped(cap)
        runs[cap], solver = _own_box_run(ctx, oracle, name, preset)
        ll = solver.last_launch()
        assert ll["lanes_per_problem"] == 16 and 16 * ll["elems_per_lane"] == cases.exact_width(case["n"]), ll
        if cap is None:
            assert ll["blocks"] == -(-cases.B // 4), ll            # one problem per segment
        else:
            assert ll["blocks"] == cap and cases.B >= 3 * cap * 4 and cases.B % 4 != 0, ll
        cases.same_bits(runs[cap], twin, "%s %s cap=%s vs twin" % (name, preset, cap))
        assert ((runs[cap][0] >= lower) & (runs[cap][0] <= upper)).all()
    cases.same_bits(runs[CAP], runs[None], "%s %s capped vs uncapped" % (name, preset))


# ---- 5 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exact_n32_m5", "relaxed_n32_m5"])
def test_one_box_in_every_row_equals_the_shared_entry(gpu_solver_factory, oracle, name):
    case = cases.BY_NAME[name]
    ctx = gpu_solver_factory().ctx
    x0 = cases.inputs(case)[0]
    lo, hi = np.full(case["n"], -1.5), np.full(case["n"], 0.8)
    for preset in ("default", "parity"):
        shared = _solver(ctx, oracle, case, preset)
        shared.SetBounds(lo, hi)
        want = _run(shared, case, x0)
        own = _solver(ctx, oracle, case, preset)
        own.SetBoundsPerProblem(np.tile(lo, (cases.B, 1)), np.tile(hi, (cases.B, 1)))
        got = _run(own, case, x0)
        assert own.last_arithmetic() == shared.last_arithmetic()
        assert {k: v for k, v in own.last_launch().items()} == {k: v for k, v in shared.last_launch().items()}
        cases.same_bits(got, want, "%s %s own rows vs shared box" % (name, preset))
        assert (want[0] == 0.8).any()
        own.SetBounds(lo, hi)                                      # ... and back to the shared box
        cases.same_bits(_run(own, case, x0), want, "%s %s after SetBounds" % (name, preset))


def test_default_arithmetic_follows_the_built_range(gpu_solver_factory, oracle):
    """arithmetic="default": the relaxed kernel where one is built for own boxes (n <= 32), the reference-order kernel at
    32 < n <= 64 — where the shared entry's default is the relaxed one."""
    import cppnumericalsolvers_amd as amd
    ctx = gpu_solver_factory().ctx
    for n, own_arith in ((20, "fma"), (40, "exact")):
        x0 = amd.synthetic_x0_host(8, n, "u2", seed=3)
        s = amd.BatchedLbfgsb(m=5, context=ctx)
        s.SetBounds(np.full(n, -1.5), np.full(n, 0.8))
        s.minimize(amd.Rosenbrock(), _to_dev(x0))
        assert s.last_arithmetic() == "fma"
        s.SetBoundsPerProblem(np.full((8, n), -1.5), np.full((8, n), 0.8))
        s.minimize(amd.Rosenbrock(), _to_dev(x0))
        assert s.last_arithmetic() == own_arith, n


# ---- 6 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exact_n32_m5", "relaxed_n20_m7", "exact_ridge_n8_m5"])
def test_results_do_not_depend_on_the_order_of_the_batch(capped, oracle, name):
    perm = np.random.default_rng(cases.SEED).permutation(cases.B)
    assert (perm != np.arange(cases.B)).mean() > 0.9
    ctx = capped(CAP)
    straight, _ = _own_box_run(ctx, oracle, name, "default")
    permuted, _ = _own_box_run(ctx, oracle, name, "default", rows=perm)
    cases.same_bits(permuted, tuple(a[perm] for a in straight), name + " permuted")


# ---- 7 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exact_n32_m5", "relaxed_n32_m5", "exact_n40_m7", "exact_ridge_n8_m5"])
def test_host_entry_equals_device_entry_also_in_chunks(gpu_solver_factory, oracle, monkeypatch, name):
    case = cases.BY_NAME[name]
    ctx = gpu_solver_factory().ctx
    dev, _ = _own_box_run(ctx, oracle, name, "default")
    x0, lower, upper, pp = cases.inputs(case)
    solver = _solver(ctx, oracle, case, "default")
    solver.SetBoundsPerProblem(lower, upper)
    cases.same_bits(solver.minimize_host(cases.engine_objective(case), x0, per_problem=pp), dev, name + " host entry")
    assert solver.last_launch()["blocks"] == -(-cases.B // 4)
    monkeypatch.setenv("MI355_HOST_STAGE_BYTES", str(64 << 10))    # the minimum: chunks of 64 problems at n >= 32
    chunked = solver.minimize_host(cases.engine_objective(case), x0, per_problem=pp)
    monkeypatch.delenv("MI355_HOST_STAGE_BYTES")
    if case["n"] >= 32:
        assert solver.last_launch()["blocks"] == 1                 # the last chunk: 131 - 2 x 64 = 3 problems
    cases.same_bits(chunked, dev, name + " host entry in chunks")   # the rows followed their chunk


def _raw_call(ctx, solver, case, lower, upper, stride, x0, host, lower_null=False):
    """mi355_lbfgsb_minimize_batch_boxes[_host] as the C-ABI takes it; (rc, (x, f, g, p))."""
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    B, n = x0.shape
    d = solver._desc(cases.engine_objective(case), n)
    if host:
        x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B)
        p = np.zeros(B, dtype=capi.PROGRESS_DTYPE)
        rc = ctx._lib.mi355_lbfgsb_minimize_batch_boxes_host(
            ctx.handle, C.byref(d), None if lower_null else lower.ctypes.data, upper.ctypes.data, stride, B, x0.ctypes.data,
            x.ctypes.data, f.ctypes.data, g.ctypes.data, p.ctypes.data)
        return rc, (x, f, g, p)
    lo_d, hi_d, x0_d = _to_dev(lower), _to_dev(upper), _to_dev(x0)
    x, g = torch.empty_like(x0_d), torch.empty_like(x0_d)
    f = torch.empty(B, dtype=torch.float64, device=x0_d.device)
    p = torch.empty(B * capi.PROGRESS_DTYPE.itemsize, dtype=torch.uint8, device=x0_d.device)
    rc = ctx._lib.mi355_lbfgsb_minimize_batch_boxes(
        ctx.handle, C.byref(d), None if lower_null else lo_d.data_ptr(), hi_d.data_ptr(), stride, B, x0_d.data_ptr(),
        x.data_ptr(), f.data_ptr(), g.data_ptr(), p.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, (x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p))


@pytest.mark.parametrize("name", ["exact_n32_m5", "relaxed_n32_m5"])
def test_padded_rows(gpu_solver_factory, oracle, monkeypatch, name):
    """box_stride = n + 3: the three doubles behind every row are never read (they hold NaN here)."""
    case = cases.BY_NAME[name]
    n = case["n"]
    ctx = gpu_solver_factory().ctx
    x0, lower, upper, _ = cases.inputs(case)
    pad = np.full((cases.B, 3), np.nan)
    wide_lo, wide_hi = np.ascontiguousarray(np.hstack([lower, pad])), np.ascontiguousarray(np.hstack([upper, pad]))
    solver = _solver(ctx, oracle, case, "default")
    twin = cases.twin(oracle, name, "default")
    rc, out = _raw_call(ctx, solver, case, wide_lo, wide_hi, n + 3, x0, host=False)
    assert rc == 0
    cases.same_bits(out, twin, name + " padded rows, device entry")
    monkeypatch.setenv("MI355_HOST_STAGE_BYTES", str(64 << 10))
    rc, out = _raw_call(ctx, solver, case, wide_lo, wide_hi, n + 3, x0, host=True)
    assert rc == 0
    cases.same_bits(out, twin, name + " padded rows, host entry in chunks")


def test_invalid_arguments(gpu_solver_factory, oracle):
    from cppnumericalsolvers_amd import capi
    case = cases.BY_NAME["exact_n32_m5"]
    ctx = gpu_solver_factory().ctx
    x0, lower, upper, _ = cases.inputs(case)
    solver = _solver(ctx, oracle, case, "default")
    bad = lower.copy()
    bad[77, 5] = np.nan
    with pytest.raises(ValueError, match="NaN bound"):
        solver.SetBoundsPerProblem(bad, upper)
    for lo, hi in ((bad, upper), (lower, np.where(np.isnan(bad), np.nan, upper))):
        rc, _ = _raw_call(ctx, solver, case, lo, hi, case["n"], x0, host=True)
        assert rc == capi.ERR_INVALID_ARGUMENT and b"NaN bound" in ctx._lib.mi355_lbfgs_last_error()
    for host in (False, True):
        rc, _ = _raw_call(ctx, solver, case, lower, upper, case["n"] - 1, x0, host=host)
        assert rc == capi.ERR_INVALID_ARGUMENT and b"box_stride" in ctx._lib.mi355_lbfgs_last_error()
        rc, _ = _raw_call(ctx, solver, case, lower, upper, case["n"], x0, host=host, lower_null=True)
        assert rc == capi.ERR_INVALID_ARGUMENT and b"required" in ctx._lib.mi355_lbfgs_last_error()
    solver.SetBoundsPerProblem(lower[:-1], upper[:-1])
    with pytest.raises(ValueError, match="per-problem bounds are"):
        solver.minimize(cases.engine_objective(case), _to_dev(x0))
    with pytest.raises(ValueError, match="per-problem bounds are"):
        solver.minimize_host(cases.engine_objective(case), x0)


def test_what_is_not_built_is_refused_and_launches_nothing(capped):
    """Every request outside the built range: MI355_ERR_UNSUPPORTED with a message that names the range, from the device
    and from the host entry, on a context that afterwards still has no launch on record."""
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    import svm_data
    ctx = capped(None)
    A = np.random.default_rng(1).normal(size=(12, 8))
    Y = np.random.default_rng(2).normal(size=(8, 12))
    al_params = np.concatenate([[0.0, 0.0, 1.0], np.zeros(3), np.zeros(8 + 2)])     # no constraints, one row
    requests = [   # (solver arguments, objective, n, per-problem rows, what the message says)
        (dict(m=5, linesearch="hager_zhang"), amd.Rosenbrock(), 8, None, "Hager-Zhang"),
        (dict(m=9), amd.Rosenbrock(), 8, None, "m = 9, 10"),
        (dict(m=10), amd.DiagQuadratic(np.ones(8)), 8, None, "m = 9, 10"),
        (dict(m=5), amd.Rosenbrock(), 65, None, "n > 64"),
        (dict(m=5, arithmetic="fma"), amd.Rosenbrock(), 40, None, "MI355_ARITH_FMA outside the relaxed range"),
        (dict(m=5, arithmetic="fma"), amd.SquaredErrorRidge(A, 0.05), 8, Y, "MI355_ARITH_FMA outside the relaxed range"),
        (dict(m=6), amd.SquaredErrorRidge(A, 0.05), 8, Y, "m > 5 on SquaredErrorRidge"),
        (dict(m=5), amd.Objective(capi.OBJ_AL_COMPOSITE, al_params, "composite"), 8, np.zeros((8, 1)), "augmented-Lagrangian"),
    ]
    for kw, objective, n, pp, text in requests:
        x0 = np.zeros((8, n))
        solver = amd.BatchedLbfgsb(context=ctx, **kw)
        solver.SetBoundsPerProblem(np.full((8, n), -1.0), np.full((8, n), 1.0))
        for call in (lambda: solver.minimize(objective, _to_dev(x0), per_problem=None if pp is None else _to_dev(pp)),
                     lambda: solver.minimize_host(objective, x0, per_problem=pp)):
            with pytest.raises(capi.EngineError) as e:
                call()
            assert e.value.code == capi.ERR_UNSUPPORTED and text in str(e.value) and "per-problem bounds are built for" in str(e.value), str(e.value)
    # a user objective, in the build of the library that holds one with Lbfgsb kernels (the dual SVM, id 101)
    svm = capped(None, library=os.path.join(ROOT, "cppnumericalsolvers_amd", "libmi355_lbfgs_svm.so"))
    X, y = svm_data.standardised_blobs(100, 4, seed=7)
    solver = amd.BatchedLbfgsb(m=5, context=svm)
    solver.SetBoundsPerProblem(np.zeros((4, 100)), np.ones((4, 100)))
    with pytest.raises(capi.EngineError) as e:
        solver.minimize(amd.Objective(capi.OBJ_USER_FIRST + 1, svm_data.dual_params(X, y)[0], "svm_dual"), _to_dev(np.zeros((4, 100))))
    # (the text is read from the library that refused: capi.check reports the first loaded library's last message)
    assert e.value.code == capi.ERR_UNSUPPORTED and b"user objectives" in svm._lib.mi355_lbfgs_last_error()
    # device groups take one shared box
    solver = amd.BatchedLbfgsb(m=5, context=ctx)
    solver.SetBoundsPerProblem(np.full((8, 8), -1.0), np.full((8, 8), 1.0))
    with pytest.raises(capi.EngineError) as e:
        amd.DeviceGroup.minimize_host_lbfgsb(None, solver, amd.Rosenbrock(), np.zeros((8, 8)))
    assert e.value.code == capi.ERR_UNSUPPORTED and "device groups" in str(e.value)
    for c in (ctx, svm):
        with pytest.raises(capi.EngineError, match="no solve has been launched"):
            amd.BatchedLbfgsb(context=c).last_kernel_ms()


def test_trace_of_three_problems_with_three_boxes(capped, oracle):
    """Rows 1, 70 and 129 (boxes 2, 8 and 4; under the cap the last two are reached on a later fetch): the traced
    iterates are those of the row solved alone under SetBounds with its box, and end in the twin's result."""
    import torch
    import cppnumericalsolvers_amd as amd
    name = "exact_n32_m5"
    case = cases.BY_NAME[name]
    n = case["n"]
    x0, lower, upper, _ = cases.inputs(case)
    rows = [1, 70, 129]
    assert len({tuple(lower[r]) + tuple(upper[r]) for r in rows}) == 3
    ctx = capped(CAP)
    dev = torch.device("cuda", 0)
    trace = amd.Trace(rows, capacity=512, n=n, device=dev, with_x=True, with_g=True)
    solver = _solver(ctx, oracle, case, "default")
    solver.SetBoundsPerProblem(lower, upper)
    x, f, g, p = _run(solver, case, x0, trace=trace)
    twin = cases.twin(oracle, name, "default")
    for i, row in enumerate(rows):
        rec, xs, gs = trace.history(i)
        alone = amd.Trace([0], capacity=512, n=n, device=dev, with_x=True, with_g=True)
        single = _solver(ctx, oracle, case, "default")
        single.SetBounds(lower[row], upper[row])
        _run(single, case, x0[row:row + 1], trace=alone)
        arec, axs, ags = alone.history(0)
        assert len(rec) == p["num_iterations"][row] == twin[3]["num_iterations"][row] and len(rec) >= 2
        assert rec.tobytes() == arec.tobytes() and xs.tobytes() == axs.tobytes() and gs.tobytes() == ags.tobytes(), row
        assert xs[-1].tobytes() == twin[0][row].tobytes() and gs[-1].tobytes() == twin[2][row].tobytes()
        assert rec[-1]["value"].tobytes() == twin[1][row].tobytes()


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_cpp_overload_equals_nine_single_solves():
    exe = os.path.join(ROOT, "tests", "own_box", "_build", "own_box_header_test")
    assert os.path.exists(exe), "tests/own_box/_build/own_box_header_test is missing: run __graft_entry__.build()"
    r = subprocess.run([exe, "solve"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr


# ---- 9 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.EXACT)
def test_exact_cases_against_the_reference_solver(gpu_solver_factory, oracle, reference, name):
    """x* and f* of every row against the reference's Lbfgsb<F, m> with that row's box (SetBounds), parity stopping."""
    from test_gpu_reference_and_dist import TOL
    case = cases.BY_NAME[name]
    (x, f, _, _), _ = _own_box_run(gpu_solver_factory().ctx, oracle, name, "parity")
    x0, lower, upper, pp = cases.inputs(case)
    recorded = cases.recorded_reference(name)
    if recorded is not None:     # a history size the reference binary does not hold: its results as recorded (tests/golden/)
        xr, fr = recorded
        print("%s: max|dx| %.3g max|df| %.3g (recorded reference)" % (name, np.abs(x - xr).max(), np.abs(f - fr).max()))
        assert np.abs(x - xr).max() <= TOL and np.abs(f - fr).max() <= TOL
        return
    blo, bhi = cases.boxes(case["n"])
    which = cases.box_of_row()
    stop = oracle.parity_stop()
    for k in range(cases.K):
        rows = np.flatnonzero(which == k)
        if case["objective"] == "squared_error_ridge":
            xr, fr, _, _ = reference.lbfgsb_ridge_minimize_batch(cases.ridge_matrix(case), cases.RIDGE_LAMBDA, pp[rows], x0[rows],
                                                                 m=case["m"], stop=stop, lower=blo[k], upper=bhi[k])
        else:
            xr, fr, _, _ = reference.lbfgsb_minimize_batch(case["objective"], x0[rows], m=case["m"], stop=stop, lower=blo[k],
                                                           upper=bhi[k])
        print("%s box %d: max|dx| %.3g max|df| %.3g" % (name, k + 1, np.abs(x[rows] - xr).max(), np.abs(f[rows] - fr).max()))
        assert np.abs(x[rows] - xr).max() <= TOL and np.abs(f[rows] - fr).max() <= TOL, (name, k + 1)
