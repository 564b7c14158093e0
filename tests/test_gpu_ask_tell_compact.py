"""The listed mode of the ask/tell handles on the device: mi355_ask_tell_compact_* / mi355_ask_tell_ids_*,
LbfgsAskTell.compact, minimize_callable(compact_every=k) and the C++ header's MinimizeBatchWithCompaction.

The oracle is the project's own: the uncompacted ask/tell path is bit for bit the persistent kernel, and the compacted
path must be bit for bit the uncompacted one — x, f, g, every progress field, the number of rounds and (Lbfgsb) the ask
counters — for Lbfgs in double and in float and for Lbfgsb under a shared box and one box per problem.  Beyond the bits:
the list is what the phase words say after every compaction, rows of problems that finished since the last compaction
are never read, a compaction that spans several workgroups keeps the order, a capped grid strides over the list, the
edges of the protocol, an objective whose per-problem data is indexed by ids, and the C++ header binary."""
import os
import subprocess

import numpy as np
import pytest

import at32_lib
import at_lib
import atb_lib

pytestmark = pytest.mark.gpu
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
B = 131
DIMS = (5, 13, 33, 65, 130)
HISTORIES = (1, 6)
EVERY = (1, 3, 16)
KINDS = ("double", "float", "shared_box", "box_per_problem")
MAPPINGS = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))
GRADIENT_STATUS = 4
PROGRAM_DIR = os.path.join(at_lib.HERE, "ask_tell_compact")


def _amd():
    import cppnumericalsolvers_amd as amd
    return amd


def _objective(objective, n):
    amd = _amd()
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


def _host(out):
    import torch
    torch.cuda.synchronize()
    x, f, g, p = out
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), _amd().progress_to_numpy(p)


def _assert_same(got, want, what):
    """bit for bit, in the precision of the results"""
    if want[0].dtype == np.float32:
        at32_lib.assert_same(got, want, what)
    else:
        at_lib.assert_same_results(got, want, what)


def _solver(factory, kind, objective, n, m, stop=None, context=None, **kw):
    """(solver, x0) of one case: Lbfgs in double / float, Lbfgsb under a shared box / one box per problem"""
    import torch
    amd = _amd()
    stop = _stop(stop or at_lib.base_stop())
    ctx = context or factory().ctx
    x0 = at_lib.starts(objective, B, n, seed=3000 * n + m)
    if kind == "double":
        return amd.BatchedLbfgs(m=m, stopping_progress=stop, arithmetic="exact", context=ctx, **kw), x0
    if kind == "float":
        return (amd.BatchedLbfgs(m=m, stopping_progress=stop, arithmetic="exact", context=ctx, dtype=torch.float32, **kw),
                np.ascontiguousarray(x0, dtype=np.float32))
    solver = amd.BatchedLbfgsb(m=m, stopping_progress=stop, arithmetic="exact", context=ctx, **kw)
    lo, hi = atb_lib.box_of(objective, n)
    if kind == "shared_box":
        solver.SetBounds(lo, hi)
    else:
        solver.SetBoundsPerProblem(*atb_lib.random_rows(lo, hi, seed=n + m))
    return solver, x0


def _handle(solver, x0d):
    amd = _amd()
    return (amd.LbfgsbAskTell if isinstance(solver, amd.BatchedLbfgsb) else amd.LbfgsAskTell)(solver, x0d)


def _uncompacted(solver, objective, x0d):
    """(results, rounds, asks or None) of minimize_callable without a list, and the handle's ask counters by hand"""
    rounds = [0]

    def fn(X):
        rounds[0] += 1
        return solver.evaluate(objective, X)

    got = _host(solver.minimize_callable(fn, x0d))
    asks = None
    if isinstance(solver, _amd().BatchedLbfgsb):
        with _handle(solver, x0d) as at:
            while at.tell(*solver.evaluate(objective, at.x)) > 0:
                pass
            asks = at.asks
    return got, rounds[0], asks


def _compacted(solver, objective, x0d, k, **kw):
    """(results, rounds, rows evaluated) of minimize_callable(compact_every=k)"""
    import torch
    rounds, rows = [0], [0]

    def fn2(X, ids):
        assert ids.dtype == torch.int64 and ids.shape == (X.shape[0],) and X.shape[0] > 0
        rounds[0] += 1
        rows[0] += X.shape[0]
        return solver.evaluate(objective, X)

    got = _host(solver.minimize_callable(fn2, x0d, compact_every=k, **kw))
    return got, rounds[0], rows[0]


def _drive_listed(at, evaluate, k, before_tell=None, max_rounds=100000):
    """the loop of minimize_callable(compact_every=k) by hand; before_tell(at, f, g): a hook between the evaluation
    and the tell.  Returns (rounds, the sequence of listed)"""
    rounds, listed = 0, []
    while True:
        listed.append(at.compact())
        if listed[-1] == 0:
            return rounds, listed
        for _ in range(k):
            f, g = evaluate(at.x)
            if before_tell is not None:
                before_tell(at, f, g)
            rounds += 1
            assert rounds < max_rounds, "the batch did not finish"
            if at.tell(f, g) == 0:
                break


# ---- same bits -------------------------------------------------------------------------------------------------------------
_reference = {}


def _reference_of(factory, kind, objective, n, m):
    """persistent kernel and uncompacted ask/tell of one case, computed once and shared by its three k"""
    import torch
    key = (kind, objective, n, m)
    if key not in _reference:
        solver, x0 = _solver(factory, kind, objective, n, m)
        x0d = torch.from_numpy(x0).to(solver.device)
        obj = _objective(objective, n)
        persistent = _host(solver.minimize(obj, x0d))
        plain, rounds, asks = _uncompacted(solver, obj, x0d)
        _assert_same(plain, persistent, "uncompacted ask/tell vs persistent kernel: %s" % (key,))
        _reference[key] = (solver, x0d, obj, persistent, plain, rounds, asks)
    return _reference[key]


def _cases():
    for kind in KINDS:
        for objective in ("rosenbrock", "diag_quadratic"):
            for n in DIMS:
                if kind in ("shared_box", "box_per_problem") and n > 64:
                    continue   # (Lbfgsb ask/tell is built for n <= 64, m <= 8)
                for m in HISTORIES:
                    yield kind, objective, n, m


@pytest.mark.parametrize("k", EVERY)
@pytest.mark.parametrize("kind,objective,n,m", list(_cases()))
def test_compacted_loop_has_the_bits_of_the_uncompacted_one(gpu_solver_factory, kind, objective, n, m, k):
    solver, x0d, obj, persistent, plain, rounds, asks = _reference_of(gpu_solver_factory, kind, objective, n, m)
    what = "%s %s n=%d m=%d compact_every=%d" % (kind, objective, n, m, k)
    got, got_rounds, rows = _compacted(solver, obj, x0d, k)
    _assert_same(got, plain, "compacted vs uncompacted: " + what)
    _assert_same(got, persistent, "compacted vs persistent kernel: " + what)
    assert got_rounds == rounds, what
    assert rows <= B * rounds
    if asks is not None:
        with _handle(solver, x0d) as at:
            by_hand, _ = _drive_listed(at, lambda X: solver.evaluate(obj, X), k)
            assert at.asks == asks, what
            assert by_hand == rounds
            _assert_same(_host(at.results()), plain, "by hand: " + what)


@pytest.mark.parametrize("W,E", MAPPINGS)
@pytest.mark.parametrize("n", [13, 130])
@pytest.mark.parametrize("kind", ["double", "float"])
def test_every_built_mapping(gpu_solver_factory, kind, n, W, E):
    import torch
    if W * E < n:
        return   # (this mapping does not cover n: refused at creation, tests/test_gpu_ask_tell.py)
    solver, x0 = _solver(gpu_solver_factory, kind, "rosenbrock", n, 6, lanes_per_problem=W, elems_per_lane=E)
    x0d = torch.from_numpy(x0).to(solver.device)
    obj = _amd().Rosenbrock()
    persistent = _host(solver.minimize(obj, x0d))
    plain, rounds, _ = _uncompacted(solver, obj, x0d)
    got, got_rounds, _ = _compacted(solver, obj, x0d, 1)
    ll = solver.last_launch()
    assert (ll["lanes_per_problem"], ll["elems_per_lane"]) == (W, E)
    what = "%s n=%d %dx%d" % (kind, n, W, E)
    _assert_same(got, plain, what)
    _assert_same(got, persistent, what + " vs persistent kernel")
    assert got_rounds == rounds


# ---- the list is right -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_list_is_what_the_phase_words_say(gpu_solver_factory, kind):
    """a handle compacted before every round beside an uncompacted one driven in lockstep"""
    import torch
    n, m = 33, 6
    solver, x0 = _solver(gpu_solver_factory, kind, "rosenbrock", n, m)
    x0d = torch.from_numpy(x0).to(solver.device)
    obj = _amd().Rosenbrock()
    listed_seen, active_seen = [], [B]
    with _handle(solver, x0d) as at, _handle(solver, x0d) as plain:
        assert at.ids is None
        ptr = at.x.data_ptr()
        for rounds in range(100000):
            listed = at.compact()
            listed_seen.append(listed)
            ids = at.ids.cpu().numpy()
            status = _host(at.results())[3]["status"]
            assert np.array_equal(ids, np.nonzero(~(status > 0))[0]), rounds
            assert ids.shape == (listed,) and np.all(np.diff(ids) > 0)
            assert at.x.shape == (listed, n) and (listed == 0 or at.x.data_ptr() == ptr)
            want_rows = plain.x.cpu().numpy()[ids]
            assert at.x.cpu().numpy().tobytes() == want_rows.tobytes(), rounds
            if listed == 0:
                break
            active = at.tell(*solver.evaluate(obj, at.x))
            active_seen.append(plain.tell(*solver.evaluate(obj, plain.x)))
            assert active == active_seen[-1] == at.active
        assert listed_seen == active_seen
        assert listed_seen[0] == B and listed_seen[-1] == 0 and len(set(listed_seen)) > 3
        _assert_same(_host(at.results()), _host(plain.results()), "lockstep " + kind)


# ---- stale rows are never read ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_rows_of_problems_finished_since_the_last_compaction_are_never_read(gpu_solver_factory, kind):
    import torch
    n, m, k = 33, 6, 5
    solver, x0 = _solver(gpu_solver_factory, kind, "rosenbrock", n, m)
    x0d = torch.from_numpy(x0).to(solver.device)
    obj = _amd().Rosenbrock()
    plain, rounds, _ = _uncompacted(solver, obj, x0d)
    poisoned = [0]

    def poison(at, f, g):
        status = torch.from_numpy(_host(at.results())[3]["status"]).to(solver.device)
        stale = status[at.ids] > 0
        poisoned[0] += int(stale.sum())
        f[stale] = float("nan")
        g[stale] = float("nan")

    with _handle(solver, x0d) as at:
        got_rounds, listed = _drive_listed(at, lambda X: solver.evaluate(obj, X), k, before_tell=poison)
        got = _host(at.results())
    _assert_same(got, plain, "NaN over stale rows, " + kind)
    assert got_rounds == rounds
    assert poisoned[0] > 0, "no problem finished between two compactions: the case shows nothing"


# ---- compaction across workgroups ------------------------------------------------------------------------------------------
def test_compaction_across_workgroups(gpu_solver_factory):
    """1031 problems, the first 300 at the minimiser.  There the first search is refused at once (g = 0): round 1 leaves
    them in the phase that wants no evaluation — still listed — and round 2 finishes them.  The compaction after round 2
    then has four whole workgroups (64 list entries each) that keep nothing and one that straddles entry 300."""
    import torch
    amd = _amd()
    Bw, n, m, first = 1031, 5, 6, 300
    x0 = at_lib.starts("diag_quadratic", Bw, n, seed=1031)
    x0[:first] = 0.0
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(at_lib.base_stop()))
    x0d = torch.from_numpy(x0).to(solver.device)
    obj = _objective("diag_quadratic", n)
    persistent = _host(solver.minimize(obj, x0d))
    assert np.all(persistent[3]["num_iterations"][:first] == 1) and persistent[3]["num_iterations"][first:].min() > 1
    plain, rounds, _ = _uncompacted(solver, obj, x0d)
    _assert_same(plain, persistent, "uncompacted vs persistent kernel")
    with amd.LbfgsAskTell(solver, x0d) as at:
        assert at.compact() == Bw
        at.tell(*solver.evaluate(obj, at.x))
        assert at.compact() == Bw and np.array_equal(at.ids.cpu().numpy(), np.arange(Bw))   # no evaluation wanted: listed
        at.tell(*solver.evaluate(obj, at.x))
        assert at.compact() == Bw - first
        ids = at.ids.cpu().numpy()
        assert ids[0] == first and np.array_equal(ids, np.arange(first, Bw))
        got_rounds, _ = _drive_listed(at, lambda X: solver.evaluate(obj, X), 1)
        got = _host(at.results())
    _assert_same(got, plain, "B = 1031")
    assert got_rounds + 2 == rounds
    by_loop, loop_rounds, rows = _compacted(solver, obj, x0d, 1)
    _assert_same(by_loop, plain, "B = 1031, minimize_callable")
    assert loop_rounds == rounds and rows < Bw * rounds


# ---- capped grid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_capped_grid_of_one_workgroup(monkeypatch, gpu_solver_factory, kind):
    """one workgroup strides over the whole list (gpu_solver_factory is asked for first, so that the session's shared
    context is never created under the cap)"""
    import torch
    amd = _amd()
    n, m = 33, 6
    solver, x0 = _solver(gpu_solver_factory, kind, "rosenbrock", n, m)
    x0d = torch.from_numpy(x0).to(solver.device)
    obj = amd.Rosenbrock()
    plain, rounds, _ = _uncompacted(solver, obj, x0d)
    monkeypatch.setenv(CAP_ENV, "1")
    ctx = amd.Context(0)
    monkeypatch.delenv(CAP_ENV, raising=False)
    try:
        capped, _ = _solver(gpu_solver_factory, kind, "rosenbrock", n, m, context=ctx)
        got, got_rounds, _ = _compacted(capped, obj, x0d, 1)
        assert capped.last_launch()["blocks"] == 1
    finally:
        ctx.close()
    _assert_same(got, plain, "one workgroup, " + kind)
    assert got_rounds == rounds


# ---- edges -----------------------------------------------------------------------------------------------------------------
def _tell_until_some_have_finished(at, solver, obj, limit=5000):
    """rounds until some, not all, of the batch have finished"""
    for _ in range(limit):
        active = at.tell(*solver.evaluate(obj, at.x))
        if active < at.B:
            assert active > 0, "the whole batch finished in one round: the case shows nothing"
            return active
    raise AssertionError("no problem finished within %d rounds" % limit)


@pytest.mark.parametrize("kind", KINDS)
def test_compact_before_the_first_tell_and_twice_in_a_row(gpu_solver_factory, kind):
    import torch
    solver, x0 = _solver(gpu_solver_factory, kind, "rosenbrock", 13, 6)
    x0d = torch.from_numpy(x0).to(solver.device)
    obj = _amd().Rosenbrock()
    with _handle(solver, x0d) as at:
        assert at.ids is None and at.x.shape == (B, 13)
        assert at.compact() == B
        assert np.array_equal(at.ids.cpu().numpy(), np.arange(B)) and at.ids.dtype == torch.int64
        assert torch.equal(at.x, x0d)
        _tell_until_some_have_finished(at, solver, obj)
        first = at.compact()
        ids, x = at.ids.clone(), at.x.clone()
        assert 0 < first < B
        assert at.compact() == first
        assert torch.equal(at.ids, ids) and at.x.cpu().numpy().tobytes() == x.cpu().numpy().tobytes()
        assert at.active == first


@pytest.mark.parametrize("count", [1, 0])
def test_batches_of_one_and_none(gpu_solver_factory, count):
    import torch
    amd = _amd()
    solver = gpu_solver_factory(m=6, stopping_progress=_stop(at_lib.base_stop()))
    x0d = torch.from_numpy(at_lib.starts("rosenbrock", count, 13, seed=5)).to(solver.device)
    obj = amd.Rosenbrock()
    calls = [0]

    def fn2(X, ids):
        calls[0] += 1
        assert X.shape == (1, 13) and ids.tolist() == [0]
        return solver.evaluate(obj, X)

    got = _host(solver.minimize_callable(fn2, x0d, compact_every=3))
    if count == 0:
        assert calls[0] == 0 and got[0].shape == (0, 13)
        with amd.LbfgsAskTell(solver, x0d) as at:
            assert at.compact() == 0 and at.ids.shape == (0,) and at.x.shape == (0, 13)
            assert at.tell(x0d[:, 0], x0d) == 0
        return
    want = _host(solver.minimize(obj, x0d))
    at_lib.assert_same_results(got, want, "B = 1")
    assert calls[0] >= int(want[3]["nfev"][0])


@pytest.mark.parametrize("kind", ["double", "float", "shared_box"])
def test_a_batch_that_finishes_in_one_round_lists_nothing(gpu_solver_factory, kind):
    """every problem starts at Rosenbrock's minimiser: no search is run, and the batch finishes in the same round"""
    import torch
    solver, x0 = _solver(gpu_solver_factory, kind, "rosenbrock", 13, 6)
    if kind == "shared_box":
        solver.SetBounds(np.full(13, -2.0), np.full(13, 2.0))   # (the minimiser inside the box)
    x0d = torch.ones_like(torch.from_numpy(x0)).to(solver.device)[:9].contiguous()
    obj = _amd().Rosenbrock()
    with _handle(solver, x0d) as at:
        assert at.compact() == 9
        active = 9
        for _ in range(4):
            if active > 0:
                active = at.tell(*solver.evaluate(obj, at.x))
        assert active == 0
        before = _host(at.results())
        assert np.all(before[3]["status"] > 0)
        assert at.compact() == 0 and at.x.shape == (0, 13) and at.ids.shape == (0,)
        empty_f = torch.empty(0, dtype=x0d.dtype, device=solver.device)
        empty_g = torch.empty(0, 13, dtype=x0d.dtype, device=solver.device)
        assert at.tell(empty_f, empty_g) == 0 and at.active == 0
        assert at.compact() == 0
        _assert_same(_host(at.results()), before, "after the empty tell, " + kind)


@pytest.mark.parametrize("kind", KINDS)
def test_tell_checks_its_rows_against_the_list(gpu_solver_factory, kind):
    import torch
    solver, x0 = _solver(gpu_solver_factory, kind, "rosenbrock", 13, 6)
    x0d = torch.from_numpy(x0).to(solver.device)
    obj = _amd().Rosenbrock()
    with _handle(solver, x0d) as at:
        at.compact()
        _tell_until_some_have_finished(at, solver, obj)
        listed = at.compact()
        assert 0 < listed < B
        f, g = solver.evaluate(obj, x0d)
        with pytest.raises(ValueError):
            at.tell(f, g)
        with pytest.raises(ValueError):
            at.tell(f[:listed], g)
        assert at.tell(*solver.evaluate(obj, at.x)) <= listed


def test_non_default_stream(gpu_solver_factory):
    import torch
    solver, x0 = _solver(gpu_solver_factory, "double", "rosenbrock", 33, 6)
    x0d = torch.from_numpy(x0).to(solver.device)
    obj = _amd().Rosenbrock()
    plain, rounds, _ = _uncompacted(solver, obj, x0d)
    stream = torch.cuda.Stream(device=solver.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got, got_rounds, _ = _compacted(solver, obj, x0d, 3)
    _assert_same(got, plain, "non-default stream")
    assert got_rounds == rounds


def test_max_rounds_exceeded_raises(gpu_solver_factory):
    import torch
    solver = gpu_solver_factory(m=6, stopping_progress=_stop(at_lib.base_stop()))
    x0d = torch.from_numpy(at_lib.starts("rosenbrock", 9, 8, seed=1)).to(solver.device)
    with pytest.raises(RuntimeError, match="still active after max_rounds = 3"):
        solver.minimize_callable(lambda X, ids: solver.evaluate(_amd().Rosenbrock(), X), x0d, max_rounds=3,
                                 compact_every=2)
    with pytest.raises(ValueError):
        solver.minimize_callable(lambda X, ids: solver.evaluate(_amd().Rosenbrock(), X), x0d, compact_every=0)


# ---- per-problem data through ids ------------------------------------------------------------------------------------------
def test_value_only_objective_with_per_problem_data_indexed_by_ids(gpu_solver_factory):
    """The inputs, the stop and the check of tests/test_gpu_ask_tell.py::test_value_only_objective_with_per_problem_data
    (f_b(x) = 1/2 ||A_b x - y_b||^2 + 1/2 lambda ||x||^2, differentiated by autograd; ||x - x*|| <= ||g(x)|| / lambda),
    with the data of the listed problems picked by ids."""
    import torch
    from cppnumericalsolvers_amd import capi
    Bv, rows, n, lam = 257, 12, 5, 0.1
    rng = np.random.default_rng(20261019)
    A, y = rng.normal(size=(Bv, rows, n)), 0.01 * rng.normal(size=(Bv, rows))
    stop = capi.default_stop()
    stop.num_iterations, stop.x_delta, stop.f_delta, stop.past = 500, 0.0, 0.0, 0
    stop.gradient_norm, stop.gradient_norm_relative = 1e-8, 0
    solver = gpu_solver_factory(m=10, stopping_progress=stop)
    Ad, yd = torch.from_numpy(A).to(solver.device), torch.from_numpy(y).to(solver.device)
    seen = dict(rounds=0, rows=0, plain_rounds=0)

    def value(X, ids):
        seen["rounds"] += 1
        seen["rows"] += X.shape[0]
        r = torch.einsum("brn,bn->br", Ad[ids], X) - yd[ids]
        return 0.5 * (r * r).sum(dim=1) + 0.5 * lam * (X * X).sum(dim=1)

    def value_all(X):
        seen["plain_rounds"] += 1
        return value(X, torch.arange(Bv, device=solver.device))

    x0d = torch.zeros(Bv, n, dtype=torch.float64, device=solver.device)
    x, f, g, p = _host(solver.minimize_callable(value, x0d, max_rounds=2000, compact_every=4))
    rounds, rows_seen = seen["rounds"], seen["rows"]
    plain = _host(solver.minimize_callable(value_all, x0d, max_rounds=2000))
    assert np.all(p["status"] == GRADIENT_STATUS), np.unique(p["status"], return_counts=True)
    assert np.array_equal(p["status"], plain[3]["status"])
    print("rows evaluated: %d of %d (%d rounds of %d problems)" % (rows_seen, Bv * rounds, rounds, Bv))
    assert rows_seen < Bv * rounds
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


def test_quadratic_with_per_problem_centres_indexed_by_ids(gpu_solver_factory):
    """f_b(x) = 1/2 sum_i a_i (x_i - c_{b,i})^2, value only, c [B, n] picked as c[ids]: the minimiser is c_b, and
    g = a (x - c) gives |x_i - c_{b,i}| <= ||g||_inf / min(a) at the gradient stop"""
    import torch
    from cppnumericalsolvers_amd import capi
    a, c, x0 = (v.astype(np.float64) for v in at32_lib.quadratic_inputs())
    tau = 1e-8
    stop = capi.default_stop()
    stop.num_iterations, stop.x_delta, stop.f_delta, stop.past = 200, 0.0, 0.0, 0
    stop.gradient_norm, stop.gradient_norm_relative = tau, 0
    solver = gpu_solver_factory(m=at32_lib.QUAD_M, stopping_progress=stop)
    ad, cd = torch.from_numpy(a).to(solver.device), torch.from_numpy(c).to(solver.device)
    seen = dict(rounds=0, rows=0)

    def value(X, ids):
        seen["rounds"] += 1
        seen["rows"] += X.shape[0]
        d = X - cd[ids]
        return 0.5 * (ad * d * d).sum(dim=1)

    x, f, g, p = _host(solver.minimize_callable(value, torch.from_numpy(x0).to(solver.device), compact_every=2,
                                                max_rounds=2000))
    assert np.all(p["status"] == GRADIENT_STATUS), np.unique(p["status"], return_counts=True)
    assert float(np.abs(x - c).max()) <= tau / a.min() * (1.0 + 1e-6)
    assert seen["rows"] < at32_lib.B * seen["rounds"]


# ---- the C++ header --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["atc_header_test", "atc_header_test_noexcept"])
def test_cpp_header_binary_matches_the_persistent_kernel(gpu_solver_factory, binary):
    import torch
    amd = _amd()
    path = os.path.join(PROGRAM_DIR, "_build", binary)
    assert os.access(path, os.X_OK), "%s is not built (run __graft_entry__.build())" % path
    out = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    n, m, Bc = 5, 6, 37
    x0 = np.array([[1.0 if b % 9 == 0 else ((1.0 if j % 2 else -1.2) + 0.03125 * b) for j in range(n)]
                   for b in range(Bc)])
    solver = gpu_solver_factory(m=m, stopping_progress=_stop(at_lib.base_stop()))
    x, f, g, p = _host(solver.minimize(amd.Rosenbrock(), torch.from_numpy(x0).to(solver.device)))

    def hexes(a):
        return [format(int(v), "016x") for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]

    lines = out.stdout.splitlines()
    summary = {w[1]: (int(w[2]), int(w[4]), int(w[6])) for w in (line.split() for line in lines) if w[0] == "rounds"}
    assert sorted(summary) == ["k1", "k4"], out.stdout
    assert summary["k1"][0] == summary["k4"][0], "the number of rounds depends on compact_every"
    for tag in ("k1", "k4"):
        rounds, rows_seen, all_rows = summary[tag]
        assert all_rows == rounds * Bc and rows_seen < all_rows
        rows = [line.split() for line in lines if line.startswith(tag + " ")]
        assert len(rows) == Bc, out.stdout
        evaluated = 0
        for b, w in enumerate(rows):
            want = ([tag, str(b), "status", str(p["status"][b]), "iterations", str(p["num_iterations"][b]), "nfev",
                     str(p["nfev"][b]), "evaluated", w[9], "f"] + hexes(f[b]) + ["x"] + hexes(x[b]))
            assert w == want, (tag, b)
            # a problem is evaluated while it is listed: at least its nfev evaluations, at most every round
            assert int(p["nfev"][b]) <= int(w[9]) <= rounds, (tag, b, w[9])
            evaluated += int(w[9])
        assert evaluated == rows_seen
    assert summary["k1"][1] <= summary["k4"][1]
