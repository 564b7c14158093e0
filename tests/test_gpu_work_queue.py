"""The work queue of the persistent solve kernels under a capped grid: what a wavefront segment computes on its second
and later fetches.

Every solve kernel takes problems from an atomic queue and resets its running state in place before the next one.
With one problem per resident segment (every small-batch test) that reset never runs.  MI355_DEBUG_SOLVE_BLOCKS, read
once when a context is created, caps the resident grid of every persistent launch; with 1 to 3 workgroups a batch of a
few hundred mixed problems makes every segment fetch many times, long solves after short ones and ordinary ones after
degenerate ones.  Each capped test first proves that it is not vacuous (`_assert_refetches`): the launch had exactly
`cap` workgroups, the batch holds at least four problems per resident segment, and — where a wavefront holds more than
one segment — the batch is not a multiple of the segments of a wavefront, so the last wavefront's segments leave the
loop at different times.

1. TrustRegionNewton (csrc/trust_region_kernel.hpp).  The oracle is the CPU twin in device order, which solves each row
   on its own: a queue or reset bug is a bit difference.
   a  mixed Rosenbrock batches (rows of exact ones and of 1e100 spliced in) at every padded width and its boundaries,
      two over-wide mappings, presets parity and default (plateau ring), caps 1 and 3 and the uncapped grid: x, f, g and
      every progress field bitwise the twin's, capped == uncapped
   b  the same device results against the twin in REFERENCE order (pinned to the reference bit for bit by
      tests/test_trust_region_twin.py).  Bounds: parity preset f and x within 1e-6, status equal or both in {2, 4};
      default preset f within 1e-6, both statuses in {3, 4} on the random rows, equal on the spliced rows; only the
      spliced overflow rows (f = inf on both sides) are left out of the f / x comparison.  Where the bounds come from —
      measured on the CPU, reference order against device order, same generator, 600 rows at n = 7, 12, 32 and 300 rows
      at n = 64: max |dx| 5.7e-8, max |df| 2.2e-15 under parity; 1 to 3 % of the rows end by x_delta (2) in one order and
      by the gradient test (4) in the other, no other status pair occurs; under default max |df| 1.5e-7 (x moves by up
      to 6e-4 there: a loose stop fires an iteration earlier or later).  n = 1: the chained Rosenbrock function has no
      term, every row stalls at once with status 2 — there every row counts as a spliced (degenerate) row: equal status.
   c  order independence: a batch and a seeded permutation of it under cap 1 permute bitwise (needs no oracle)
   d  condition_hessian on: n = 4 with the limit 50 (rows stopped with status 5 followed by rows that converge) and
      1e4, n = 64 at W = 64 (the largest LDS footprint the launch takes) with the limit 1e5
   e  DiagQuadratic n = 12: the golden file's indefinite set with num_iterations = 25, and its convex set
   f  the quartic double well as a user functor (libmi355_lbfgs_tr.so), 1000 starts and the degenerate start 0
   g  a Trace on two rows that a segment reaches on a later fetch == the trace of the row solved alone
   h  minimize_host == minimize on a capped batch
   i  the full uncapped W = 8 grid with more than two problems per resident segment (plateau-ring scratch check passes)
2. One capped batch (caps 1 and 2) per family of the other persistent kernels, through the public solvers, bitwise the
   family's oracle twin called as the neighbouring modules call it, and bitwise the same solver on an uncapped context:
   general Lbfgs (More-Thuente, exact, default preset), Lbfgs with Hager-Zhang exact and fused, Second-mode Lbfgs with
   condition_hessian on, dense Bfgs (n = 32 and n = 7), exact and relaxed-algebra Lbfgsb in a box that puts start
   coordinates on a bound, the workgroup kernel for n > 256, the ridge kernel on the matrix cores, and the lean kernel
   (against the general kernel and the twin).
   The augmented-Lagrangian loops (the fused loop resets its outer-loop state inside these kernels; the lock-step loop
   launches them through problem_map / count_dev) have a module of their own: tests/test_gpu_auglag_queue.py.
   NOT covered here: the ridge Gram pre-pass (not a persistent kernel; its solve is the general Lbfgs kernel).
"""
import os

import numpy as np
import pytest

import tr_cases
import tr_lib as T
import tr_queue as Q

pytestmark = pytest.mark.gpu
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
GOLDEN = {c["name"]: c for c in tr_cases.load_cases()}
SEED = 20261016


@pytest.fixture
def capped(monkeypatch, gpu_solver_factory):
    """capped(cap, library=None): a FRESH context created with the resident grid capped to `cap` workgroups (None: a
    fresh uncapped context).  (gpu_solver_factory is asked for first, so that the session's shared context can never be
    created while the variable is set.)"""
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


def _run(solver, objective, x0, per_problem=None, trace=None):
    import torch
    import cppnumericalsolvers_amd as amd
    x, f, g, p = solver.minimize(objective, _to_dev(x0), trace=trace,
                                 per_problem=None if per_problem is None else _to_dev(per_problem))
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)


def _segments(ll):
    """(segments of a wavefront, problem slots of a workgroup) of a launch."""
    lanes = ll["lanes_per_problem"]
    if lanes > 64:                      # the workgroup kernel: one problem per workgroup
        return 1, 1
    return 64 // lanes, (64 // lanes) * (ll["threads"] // 64)


def _assert_refetches(ll, cap, B):
    per_wave, per_block = _segments(ll)
    assert ll["blocks"] == cap, (ll, cap)                       # the cap reached this launch
    assert B >= 4 * cap * per_block, (B, cap, per_block)        # the average segment fetches four times or more
    assert per_wave == 1 or B % per_wave != 0, (B, per_wave)    # a ragged last wavefront


def _assert_same_bits(a, b, what):
    diff = Q.same_bits(a, b)
    assert diff is None, "%s: %s" % (what, diff)


# ======================================================================================================================
# 1. TrustRegionNewton
# ======================================================================================================================
def _tr_stop(rec):
    from cppnumericalsolvers_amd import capi
    s = capi.Stop()
    for k in T.STOP_DTYPE.names:
        setattr(s, k, rec[k][0].item())
    return s


def _tr_solver(ctx, stop, config=None, lanes=0, condition=0.0):
    import cppnumericalsolvers_amd as amd
    kw = {} if config is None else {k: config[k][0].item() for k in T.CONFIG_FIELDS}
    return amd.BatchedTrustRegionNewton(stopping_progress=_tr_stop(stop), context=ctx, lanes_per_problem=lanes,
                                        condition_hessian=condition, **kw)


def _tr_capped(ctx, cap, objective, x0, stop, W, config=None, condition=0.0, trace=None):
    """One capped trust-region solve on W lanes per problem, proven to re-fetch."""
    n = x0.shape[1]
    solver = _tr_solver(ctx, stop, config, lanes=0 if W == Q.padded_width(n) else W, condition=condition)
    out = _run(solver, objective, x0, trace=trace)
    ll = solver.last_launch()
    assert ll["lanes_per_problem"] == W, ll
    if cap is not None:
        _assert_refetches(ll, cap, x0.shape[0])
    return out, ll


# (n, W, B): every padded width with its boundaries, then the over-wide mappings.  B >= 4 x 3 workgroups x 64 / W
# segments, never a multiple of 64 / W; the shapes on 64 lanes (one problem per wavefront) take a smaller batch
TR_SHAPES = [(1, 8, 203), (7, 8, 203), (8, 8, 203), (9, 16, 131), (16, 16, 131), (17, 32, 67), (32, 32, 67), (33, 64, 29),
             (63, 64, 29), (64, 64, 29), (7, 64, 29), (12, 32, 67)]
_tr_cache = {}


def _tr_mixed(n, W, B):
    return Q.mixed_rosenbrock_batch(n, B, SEED + 100 * n + W)


def _tr_cap1(capped, n, W, B, preset):
    """The cap-1 device result of a mixed batch (kept for the tests that compare it with something else)."""
    import cppnumericalsolvers_amd as amd
    key = (n, W, B, preset)
    if key not in _tr_cache:
        x0 = _tr_mixed(n, W, B)[0]
        _tr_cache[key] = _tr_capped(capped(1), 1, amd.Rosenbrock(), x0, T.make_stop(**T.STOP_PRESETS[preset]), W)[0]
    return _tr_cache[key]


@pytest.mark.parametrize("preset", ["parity", "default"])
@pytest.mark.parametrize("n,W,B", TR_SHAPES)
def test_tr_mixed_batches_equal_twin_under_every_grid(capped, gpu_solver_factory, n, W, B, preset):
    """1a.  Caps 1 and 3 and the uncapped grid: bitwise the device-order twin, and each other."""
    import cppnumericalsolvers_amd as amd
    x0, ones, big = _tr_mixed(n, W, B)
    stop = T.make_stop(**T.STOP_PRESETS[preset])
    twin = Q.twin_solve(T.ROSENBROCK, x0, None, stop, T.make_config(), order=T.DEVICE_ORDER, W=W)
    if n >= 2:   # the batch is what it is meant to be: stalls, overflows, and solves of very different lengths
        assert (twin[3]["status"][ones] == 2).all() and (twin[3]["nfev"][ones] == 22).all()
        assert np.isinf(twin[1][big]).all()
        it = np.delete(twin[3]["num_iterations"], np.concatenate([ones, big]))
        assert it.min() <= 12 and it.max() >= 4 * it.min()
    runs = {}
    for cap in (1, 3, None):
        ctx = capped(cap) if cap else gpu_solver_factory().ctx
        runs[cap], ll = _tr_capped(ctx, cap, amd.Rosenbrock(), x0, stop, W)
        if cap is None:
            assert ll["blocks"] == -(-B // (64 // W))       # the uncapped grid: one problem per segment
        _assert_same_bits(runs[cap], twin, "n=%d W=%d %s cap=%s vs twin" % (n, W, preset, cap))
    _tr_cache[(n, W, B, preset)] = runs[1]
    for cap in (1, 3):
        _assert_same_bits(runs[cap], runs[None], "n=%d W=%d %s cap=%d vs uncapped" % (n, W, preset, cap))


@pytest.mark.parametrize("preset", ["parity", "default"])
@pytest.mark.parametrize("n,W,B", TR_SHAPES)
def test_tr_capped_batches_within_the_bound_of_the_reference_order(capped, n, W, B, preset):
    """1b.  The cap-1 device results against the twin in the REFERENCE's summation order (module docstring: where the
    bounds and the status rule come from).  No row is left out but the spliced overflow rows."""
    x0, ones, big = _tr_mixed(n, W, B)
    x, f, g, p = _tr_cap1(capped, n, W, B, preset)
    rx, rf, rg, rp = Q.twin_solve(T.ROSENBROCK, x0, None, T.make_stop(**T.STOP_PRESETS[preset]), T.make_config(),
                                  order=T.REF_ORDER, W=W)
    spliced = np.zeros(B, dtype=bool)
    spliced[ones] = spliced[big] = True
    keep = np.ones(B, dtype=bool)
    if n >= 2:
        keep[big] = False
        assert np.isinf(f[big]).all() and np.isinf(rf[big]).all()
    else:
        spliced[:] = True       # n = 1: every row is degenerate (module docstring)
    ds, rs = p["status"], rp["status"]
    print("n=%d W=%d %s: max|df| %.3g max|dx| %.3g, %d of %d rows with another status" %
          (n, W, preset, np.max(np.abs(f[keep] - rf[keep])), np.max(np.abs(x[keep] - rx[keep])), int(np.sum(ds != rs)), B))
    np.testing.assert_allclose(f[keep], rf[keep], rtol=0, atol=1e-6)
    assert (ds[spliced] == rs[spliced]).all(), (ds[spliced], rs[spliced])
    if preset == "parity":
        np.testing.assert_allclose(x[keep], rx[keep], rtol=0, atol=1e-6)
        assert ((ds == rs) | (np.isin(ds, (2, 4)) & np.isin(rs, (2, 4)))).all(), (ds, rs)
    else:
        assert np.isin(ds[~spliced], (3, 4)).all() and np.isin(rs[~spliced], (3, 4)).all(), (ds, rs)


@pytest.mark.parametrize("n,W,B,preset", [(7, 8, 203, "default"), (32, 32, 67, "parity"), (12, 32, 67, "default")])
def test_tr_results_do_not_depend_on_the_order_of_the_batch(capped, n, W, B, preset):
    """1c.  A batch and a seeded permutation of it under cap 1: the results permute bitwise."""
    import cppnumericalsolvers_amd as amd
    x0 = _tr_mixed(n, W, B)[0]
    perm = np.random.default_rng(SEED + n).permutation(B)
    assert (perm != np.arange(B)).mean() > 0.9
    a = _tr_cap1(capped, n, W, B, preset)
    b, _ = _tr_capped(capped(1), 1, amd.Rosenbrock(), x0[perm], T.make_stop(**T.STOP_PRESETS[preset]), W)
    _assert_same_bits(tuple(u[perm] for u in a), b, "permuted n=%d %s" % (n, preset))


def _condition_batch(n, W, B):
    x0, ones, big = Q.mixed_rosenbrock_batch(n, B, SEED + 100 * n + W + 7)
    near = np.arange(5, B, 7)     # starts within 1e-7 of the minimiser: the gradient test fires before the condition test
    x0[near] = 1.0 + 1e-7 * np.random.default_rng(SEED + 1).uniform(-1, 1, (near.size, n))
    return x0


@pytest.mark.parametrize("n,W,B,limit,preset", [(4, 8, 203, 50.0, "default"), (4, 8, 203, 1e4, "default"),
                                                (4, 8, 203, 1e4, "parity"), (64, 64, 29, 1e5, "default"),
                                                (64, 64, 29, 1e5, "parity")])
def test_tr_condition_hessian_with_refetch(capped, gpu_solver_factory, n, W, B, limit, preset):
    """1d.  condition_hessian on: rows stopped by the condition test (status 5) followed by rows that converge, the LU's
    LDS region reused by consecutive problems; n = 64 on 64 lanes is the largest LDS footprint the launch accepts."""
    import cppnumericalsolvers_amd as amd
    x0 = _condition_batch(n, W, B)
    stop = T.make_stop(**T.STOP_PRESETS[preset])
    twin = Q.twin_solve(T.ROSENBROCK, x0, None, stop, T.make_config(), limit, order=T.DEVICE_ORDER, W=W)
    st = twin[3]["status"]
    assert np.sum(st == 5) >= 8 and np.sum(np.isin(st, (3, 4))) >= 8, np.unique(st, return_counts=True)
    assert (np.isin(st[:-1], (5,)) & np.isin(st[1:], (3, 4))).any()    # ... one right after the other in queue order
    for cap in (1, 3):
        out, ll = _tr_capped(capped(cap), cap, amd.Rosenbrock(), x0, stop, W, condition=limit)
        _assert_same_bits(out, twin, "condition n=%d limit=%g %s cap=%d" % (n, limit, preset, cap))
    out, _ = _tr_capped(gpu_solver_factory().ctx, None, amd.Rosenbrock(), x0, stop, W, condition=limit)
    _assert_same_bits(out, twin, "condition n=%d uncapped" % n)


@pytest.mark.parametrize("name", ["diag_quadratic_indefinite", "diag_quadratic_convex"])
def test_tr_diag_quadratic_with_refetch(capped, name):
    """1e.  DiagQuadratic n = 12 with the golden file's parameter sets (the indefinite one runs into its limit of 25
    iterations: every step leaves through the boundary of the region), 301 mixed starts under cap 1."""
    import cppnumericalsolvers_amd as amd
    case = GOLDEN[name]
    n, B, W = 12, 301, 16
    assert case["x0"].shape[1] == n and (name != "diag_quadratic_indefinite" or case["stop"]["num_iterations"][0] == 25)
    rng = np.random.default_rng(SEED + 5)
    x0 = rng.choice(Q.SCALES, size=B)[:, None] * rng.uniform(-1, 1, (B, n))
    x0[[0, 77, 150, B - 1]] = 0.0                     # the stationary point: the step stays zero
    twin = Q.twin_solve(T.DIAG_QUADRATIC, x0, case["params"], case["stop"], case["config"], order=T.DEVICE_ORDER, W=W)
    assert (twin[3]["status"][[0, 77, 150, B - 1]] == 2).all()
    assert (np.delete(twin[3]["status"], [0, 77, 150, B - 1]) == (1 if name.endswith("indefinite") else 4)).all()
    obj = amd.DiagQuadratic(case["params"][:n], float(case["params"][n]))
    out, _ = _tr_capped(capped(1), 1, obj, x0, case["stop"], W, config=case["config"])
    _assert_same_bits(out, twin, name)


def _library(name):
    return os.path.join(T.REPO, "cppnumericalsolvers_amd", name)


def test_tr_user_functor_with_refetch(capped):
    """1f.  The quartic double well as a user device functor, 1000 starts in [-3, 3] and the degenerate start 0 (zero
    gradient at a maximum: the solve stalls) under cap 1."""
    import cppnumericalsolvers_amd as amd
    case = GOLDEN["quartic"]
    x0 = np.concatenate([np.random.default_rng(SEED + 6).uniform(-3, 3, 1000), [0.0]])[:, None]
    x0[[3, 500]] = 0.0
    twin = Q.twin_solve(T.QUARTIC, x0, None, case["stop"], case["config"], order=T.DEVICE_ORDER, W=8)
    assert (twin[3]["status"][[3, 500, 1000]] == 2).all() and (np.delete(twin[3]["status"], [3, 500, 1000]) == 4).all()
    out, _ = _tr_capped(capped(1, library=_library("libmi355_lbfgs_tr.so")), 1, amd.Objective(100, np.zeros(0), "quartic"),
                        x0, case["stop"], 8, config=case["config"])
    _assert_same_bits(out, twin, "quartic")


def test_tr_trace_across_a_refetch(capped):
    """1g.  Traced rows that a segment can only reach on a later fetch (index >= workgroups x segments): the history
    equals, bitwise, the history of the same row solved alone, and ends with the row's progress record."""
    import torch
    import cppnumericalsolvers_amd as amd
    n, W, B = 7, 8, 203
    x0 = _tr_mixed(n, W, B)[0]
    stop = T.make_stop(**T.STOP_PRESETS["default"])
    rows = [101, B - 2]
    ctx = capped(1)
    trace = amd.Trace(rows, capacity=1024, n=n, device=torch.device("cuda", 0), with_x=True, with_g=True)
    (x, f, g, p), ll = _tr_capped(ctx, 1, amd.Rosenbrock(), x0, stop, W, trace=trace)
    assert min(rows) >= ll["blocks"] * (64 // W)
    for i, row in enumerate(rows):
        rec, xs, gs = trace.history(i)
        alone = amd.Trace([0], capacity=1024, n=n, device=torch.device("cuda", 0), with_x=True, with_g=True)
        _run(_tr_solver(ctx, stop), amd.Rosenbrock(), x0[row:row + 1], trace=alone)
        arec, axs, ags = alone.history(0)
        assert len(rec) == p["num_iterations"][row] and len(rec) > 5
        assert rec.tobytes() == arec.tobytes() and xs.tobytes() == axs.tobytes() and gs.tobytes() == ags.tobytes(), row
        last = rec[-1]
        for k in ("num_iterations", "status", "x_delta", "f_delta", "gradient_norm"):
            assert last[k].tobytes() == p[k][row].tobytes(), (row, k)
        assert last["value"].tobytes() == f[row].tobytes()
        assert xs[-1].tobytes() == x[row].tobytes() and gs[-1].tobytes() == g[row].tobytes()


def test_tr_host_entry_equals_device_entry_capped(capped):
    """1h.  minimize_host == minimize on a capped mixed batch."""
    import cppnumericalsolvers_amd as amd
    n, W, B, preset = 16, 16, 131, "default"
    x0 = _tr_mixed(n, W, B)[0]
    dev = _tr_cap1(capped, n, W, B, preset)
    solver = _tr_solver(capped(1), T.make_stop(**T.STOP_PRESETS[preset]))
    hx, hf, hg, hp = solver.minimize_host(amd.Rosenbrock(), x0)
    _assert_refetches(solver.last_launch(), 1, B)
    _assert_same_bits(dev, (hx, hf, hg, hp), "host entry")


def test_tr_full_uncapped_grid_refetches(gpu_solver_factory):
    """1i.  The whole resident W = 8 grid, more than two problems per segment, default preset (one plateau ring per
    resident segment in the context's scratch): the launch is not refused, and equals the twin bitwise."""
    import cppnumericalsolvers_amd as amd
    n, W = 7, 8
    stop = T.make_stop(**T.STOP_PRESETS["default"])
    solver = _tr_solver(gpu_solver_factory().ctx, stop)
    _run(solver, amd.Rosenbrock(), np.ones((2 * 8 * 32 * 304, n)))   # probe: more rows of ones than any grid holds
    blocks = solver.last_launch()["blocks"]
    assert blocks * 8 < 2 * 8 * 32 * 304
    B = 2 * blocks * 8 + 5
    x0, ones, big = Q.mixed_rosenbrock_batch(n, B, SEED + 9)
    out = _run(solver, amd.Rosenbrock(), x0)
    ll = solver.last_launch()
    assert ll["blocks"] == blocks and ll["lanes_per_problem"] == W and B > 2 * ll["blocks"] * 8 and B % 8 != 0
    twin = Q.twin_solve(T.ROSENBROCK, x0, None, stop, T.make_config(), order=T.DEVICE_ORDER, W=W)
    _assert_same_bits(out, twin, "full grid, B=%d on %d workgroups" % (B, blocks))


# ======================================================================================================================
# 2. the other persistent kernels
# ======================================================================================================================
FAMILY_CAPS = (1, 2)


def _engine_stop(oracle_stop):
    from cppnumericalsolvers_amd import capi
    dst = capi.Stop()
    for name, _ in oracle_stop._fields_:
        setattr(dst, name, getattr(oracle_stop, name))
    return dst


def _lbfgs_mixed_starts(oracle, n, B, seed, hostile=False):
    """Rows of the two synthetic start kinds (long solves), rows next to the minimiser (short ones), rows of exact ones
    (a stall at once) and — for the kernels whose twin is pinned on them — the non-finite and overflowing starts."""
    import cppnumericalsolvers_amd as amd
    x0 = amd.synthetic_x0_host(B, n, "std", seed=seed)
    x0[1::3] = amd.synthetic_x0_host(B, n, "u2", seed=seed)[1::3]
    rng = np.random.default_rng(seed)
    x0[2::3] = 1.0 + 0.05 * rng.uniform(-1, 1, (B, n))[2::3]
    x0[[0, B // 2, B - 1]] = 1.0
    if hostile:
        rows = np.linspace(3, B - 3, 10).astype(int)
        x0[rows] = oracle.hostile_starts(n)
    return x0


def _family(capped, uncapped_ctx, make_solver, objective, x0, per_problem=None, fields=Q.FIELDS, check_launch=None):
    """The solver on an uncapped context and under every cap: (uncapped result, launch record); the capped results are
    bitwise the uncapped one."""
    B = x0.shape[0]
    base_solver = make_solver(uncapped_ctx)
    base = _run(base_solver, objective, x0, per_problem)
    base_ll = base_solver.last_launch()
    if check_launch:
        check_launch(base_solver)
    for cap in FAMILY_CAPS:
        solver = make_solver(capped(cap))
        out = _run(solver, objective, x0, per_problem)
        ll = solver.last_launch()
        _assert_refetches(ll, cap, B)
        if check_launch:
            check_launch(solver)
        assert {k: v for k, v in ll.items() if k != "blocks"} == {k: v for k, v in base_ll.items() if k != "blocks"}
        for name, a, b in zip(("x", "f", "g"), out[:3], base[:3]):
            np.testing.assert_array_equal(a, b, err_msg="cap %d: %s" % (cap, name))
        for k in fields:
            np.testing.assert_array_equal(out[3][k], base[3][k], err_msg="cap %d: %s" % (cap, k))
    return base, base_ll


def _assert_equals_twin(dev, twin, fields=Q.FIELDS):
    for name, a, b in zip(("x", "f", "g"), dev[:3], twin[:3]):
        np.testing.assert_array_equal(a, b, err_msg=name)
    for k in fields:
        np.testing.assert_array_equal(dev[3][k], twin[3][k], err_msg=k)


def test_general_lbfgs_default_preset_capped(capped, gpu_solver_factory, oracle):
    """Lbfgs, More-Thuente, exact arithmetic, n = 32, the default preset (past = 3: the plateau ring is reused)."""
    import cppnumericalsolvers_amd as amd
    n, m, B = 32, 6, 203
    x0 = _lbfgs_mixed_starts(oracle, n, B, seed=11, hostile=True)
    stop_o = oracle.default_stop()
    make = lambda ctx: amd.BatchedLbfgs(m=m, stopping_progress=_engine_stop(stop_o), context=ctx, arithmetic="exact")
    dev, ll = _family(capped, gpu_solver_factory().ctx, make, amd.Rosenbrock(), x0)
    _assert_equals_twin(dev, oracle.minimize_batch("rosenbrock", x0, m=m, stop=stop_o, reduction="butterfly", width=32))


@pytest.mark.parametrize("arithmetic", ["exact", "fma"])
def test_lbfgs_hager_zhang_capped(capped, gpu_solver_factory, oracle, arithmetic):
    import cppnumericalsolvers_amd as amd
    n, m, B = 32, 6, 203
    x0 = _lbfgs_mixed_starts(oracle, n, B, seed=12, hostile=arithmetic == "exact")
    for stop_o in (oracle.default_stop(), oracle.parity_stop()):
        make = lambda ctx: amd.BatchedLbfgs(m=m, stopping_progress=_engine_stop(stop_o), context=ctx, arithmetic=arithmetic,
                                            linesearch="hager_zhang")
        dev, ll = _family(capped, gpu_solver_factory().ctx, make, amd.Rosenbrock(), x0,
                          check_launch=lambda s: s.last_arithmetic() == arithmetic or pytest.fail(s.last_arithmetic()))
        E = ll["elems_per_lane"]
        fused = arithmetic == "fma"
        _assert_equals_twin(dev, oracle.minimize_batch("rosenbrock", x0, m=m, stop=stop_o, linesearch="hager_zhang",
                                                       reduction="butterfly_fma" if fused else "butterfly",
                                                       width=max(32, E) if fused else 32, fma_group=E if fused else 0))


def test_second_mode_lbfgs_with_condition_hessian_capped(capped, gpu_solver_factory, oracle):
    """Second-mode Lbfgs (preconditioner from the functor's Hessian diagonal) with the condition_hessian test on: the
    Hessian and LU regions in LDS are reused by consecutive problems, some stopped by the test (status 5)."""
    import cppnumericalsolvers_amd as amd
    n, m, B, threshold = 32, 5, 203, 3e4
    rng = np.random.default_rng(31 * n + m)
    x0 = np.vstack([np.tile([-1.2, 1.0], n)[:n], rng.uniform(-2, 2, (B - 1, n))])
    x0[2::3] = 1.0 + 0.05 * rng.uniform(-1, 1, (B, n))[2::3]
    obj = amd.Rosenbrock(differentiability="second")
    make = lambda ctx: amd.BatchedLbfgs(m=m, context=ctx, arithmetic="exact", condition_hessian=threshold)
    dev, ll = _family(capped, gpu_solver_factory().ctx, make, obj, x0, fields=("status", "num_iterations", "nfev", "sum_k"))
    W, E = ll["lanes_per_problem"], ll["elems_per_lane"]
    oracle.lib().oracle_set_condition_hessian_stop(threshold)
    try:
        twin = oracle.minimize_batch("rosenbrock", x0, m=m, second_mode="functor", reduction="butterfly", width=W * E)
        co = oracle.hessian_conditions(B)
    finally:
        oracle.lib().oracle_set_condition_hessian_stop(0.0)
    assert np.all(np.abs(co - threshold) > 1e-9 * threshold)
    _assert_equals_twin(dev, twin, fields=("status", "num_iterations", "nfev", "sum_k"))
    assert np.sum(dev[3]["status"] == 5) >= 8 and np.sum(dev[3]["status"] != 5) >= 8


@pytest.mark.parametrize("ls", ["more_thuente", "hager_zhang"])
@pytest.mark.parametrize("n,B", [(32, 131), (7, 203)])
def test_dense_bfgs_capped(capped, gpu_solver_factory, oracle, n, B, ls):
    """Dense Bfgs: the inverse-Hessian approximation in LDS is reset to the identity per problem.

    The spliced non-finite starts include rows whose gradient is NaN in EVERY coordinate; at n = 32 the problem fills
    its 32 lanes, no padding lane contributes a 0 to the max-butterfly, and the norm must still be the 0 of the
    reference's `m = 0; if (m < t) m = t` fold (seg_amax, csrc/wave_primitives.hpp): the gradient test then stops the
    solve after 4 iterations, as in the twin, instead of running into the iteration limit."""
    import cppnumericalsolvers_amd as amd
    x0 = _lbfgs_mixed_starts(oracle, n, B, seed=5 * n + 1, hostile=True)
    stop_o = oracle.default_stop()
    make = lambda ctx: amd.BatchedBfgs(stopping_progress=_engine_stop(stop_o), context=ctx, linesearch=ls)
    dev, ll = _family(capped, gpu_solver_factory().ctx, make, amd.Rosenbrock(), x0)
    twin = oracle.bfgs_minimize_batch("rosenbrock", x0, stop=stop_o, reduction="butterfly", width=Q.padded_width(n),
                                      linesearch=ls)
    _assert_equals_twin(dev, twin, fields=("status", "num_iterations", "nfev"))


def _box_starts(n, B, seed):
    """Starts in [-2, 2] against the box [-1.5, 0.8]: coordinates outside start on a bound after the projection; some
    rows lie on a bound exactly, one row in a corner."""
    import cppnumericalsolvers_amd as amd
    x0 = amd.synthetic_x0_host(B, n, "u2", seed=seed)
    x0[3::11, ::2] = -1.5
    x0[5::13, 1::2] = 0.8
    x0[B // 2] = 0.8
    return x0, np.full(n, -1.5), np.full(n, 0.8)


def test_exact_lbfgsb_capped(capped, gpu_solver_factory, oracle):
    import cppnumericalsolvers_amd as amd
    n, m, B = 32, 5, 131
    x0, lo, hi = _box_starts(n, B, seed=n * 3 + 1)
    for stop_o in (oracle.lbfgsb_default_stop(), oracle.parity_stop()):
        def make(ctx):
            s = amd.BatchedLbfgsb(arithmetic="exact", m=m, stopping_progress=_engine_stop(stop_o), context=ctx)
            s.SetBounds(lo, hi)
            return s
        dev, ll = _family(capped, gpu_solver_factory().ctx, make, amd.Rosenbrock(), x0)
        _assert_equals_twin(dev, oracle.lbfgsb_minimize_batch("rosenbrock", x0, m=m, stop=stop_o, lower=lo, upper=hi,
                                                               reduction="butterfly", width=32))
        assert np.all(dev[0] <= 0.8) and np.all(dev[0] >= -1.5)


def test_fast_lbfgsb_capped(capped, gpu_solver_factory, oracle):
    import cppnumericalsolvers_amd as amd
    n, m, B = 32, 5, 131
    x0, lo, hi = _box_starts(n, B, seed=n * 3 + 2)
    tight = oracle.make_stop(num_iterations=10000, x_delta=1e-11, x_delta_violations=1, f_delta=0.0, gradient_norm=1e-8,
                             past=0)
    for stop_o in (oracle.lbfgsb_default_stop(), tight):
        def make(ctx):
            s = amd.BatchedLbfgsb(m=m, stopping_progress=_engine_stop(stop_o), context=ctx, arithmetic="fma")
            s.SetBounds(lo, hi)
            return s
        dev, ll = _family(capped, gpu_solver_factory().ctx, make, amd.Rosenbrock(), x0,
                          check_launch=lambda s: s.last_arithmetic() == "fma" or pytest.fail(s.last_arithmetic()))
        _assert_equals_twin(dev, oracle.lbfgsb_fast_minimize_batch("rosenbrock", x0, m=m, stop=stop_o, lower=lo, upper=hi))


def test_wide_kernel_capped(capped, gpu_solver_factory, oracle):
    """n > 256: one problem per workgroup, vectors and correction ring in a workspace slot that the next problem reuses."""
    import cppnumericalsolvers_amd as amd
    n, m, B = 300, 6, 21
    rng = np.random.default_rng(7 * n + m)
    x0 = np.tile([-1.2, 1.0], n)[:n] + 0.1 * rng.uniform(-1, 1, (B, n))
    x0[1::3] = 1.0 + 0.05 * rng.uniform(-1, 1, (B, n))[1::3]
    x0[[4, B - 1]] = 1.0
    for stop_o in (oracle.default_stop(), oracle.parity_stop()):
        make = lambda ctx: amd.BatchedLbfgs(m=m, stopping_progress=_engine_stop(stop_o), context=ctx)
        dev, ll = _family(capped, gpu_solver_factory().ctx, make, amd.Rosenbrock(), x0)
        assert ll["threads"] == 256 and ll["elems_per_lane"] == 2
        _assert_equals_twin(dev, oracle.minimize_batch("rosenbrock", x0, m=m, stop=stop_o, reduction="strided", width=256))


def test_ridge_matrix_core_kernel_capped(capped, gpu_solver_factory, oracle):
    """The joint-evaluation ridge kernel: sixteen problem slots per workgroup, each refilled from the queue while the
    others keep evaluating; default preset (plateau ring per slot) and parity."""
    import cppnumericalsolvers_amd as amd
    rows, n, B, m, lam = 128, 64, 203, 10, 0.1
    A, Y = amd.synthetic_ridge_host(B, rows, n, seed=rows + n + B)
    x0 = np.zeros((B, n))
    x0[1::2] = np.random.default_rng(3).uniform(-2, 2, (B, n))[1::2]
    obj = amd.SquaredErrorRidge(A, lam, matrix_cores=True)
    for stop_o in (oracle.default_stop(), oracle.parity_stop()):
        make = lambda ctx: amd.BatchedLbfgs(m=m, stopping_progress=_engine_stop(stop_o), context=ctx, arithmetic="exact")
        dev, ll = _family(capped, gpu_solver_factory().ctx, make, obj, x0, per_problem=Y)
        assert ll["threads"] == 512 and ll["lanes_per_problem"] == 32 and ll["elems_per_lane"] == 2
        _assert_equals_twin(dev, oracle.minimize_batch("squared_error_ridge_mfma", x0, m=m, stop=stop_o,
                                                       params=oracle.ridge_params(A, lam), reduction="butterfly", width=64,
                                                       per_problem=Y))


def test_lean_kernel_capped(capped, gpu_solver_factory, oracle):
    """The lean launch-specialised kernel under parity stopping: capped == uncapped == the general kernel == the twin."""
    import torch
    import cppnumericalsolvers_amd as amd
    n, m, B = 32, 6, 203
    x0 = _lbfgs_mixed_starts(oracle, n, B, seed=13)
    make = lambda ctx: amd.BatchedLbfgs(m=m, stopping_progress=amd.parity_stop(), context=ctx)
    dev, ll = _family(capped, gpu_solver_factory().ctx, make, amd.Rosenbrock(), x0,
                      check_launch=lambda s: s.last_launch()["kernel"] == "lean" or pytest.fail(str(s.last_launch())))
    assert ll["kernel"] == "lean"
    E = ll["elems_per_lane"]
    _assert_equals_twin(dev, oracle.minimize_batch("rosenbrock", x0, m=m, stop=oracle.parity_stop(),
                                                   reduction="butterfly_fma", width=max(32, E), fma_group=E))
    for cap in FAMILY_CAPS:      # the general kernel (a trace disqualifies the lean one without changing a result)
        solver = make(capped(cap))
        trace = amd.Trace([0], 4, n, torch.device("cuda", 0), with_x=False)
        general = _run(solver, amd.Rosenbrock(), x0, trace=trace)
        assert solver.last_launch()["kernel"] == "general"
        _assert_refetches(solver.last_launch(), cap, B)
        _assert_equals_twin(general, dev)
