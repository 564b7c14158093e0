"""The augmented-Lagrangian loops under a capped grid and across the hand-over: what a wavefront segment computes for a
constrained problem it fetches after it has solved another one, and what the lock-step loop's queue inputs
(problem_map, count_dev) do on a single workgroup.  (tests/test_gpu_work_queue.py does the same for the other persistent
kernels; MI355_DEBUG_SOLVE_BLOCKS, read once when a context is created, caps the resident grid.)

In the fused loop (AugLagOuterLoop inside lbfgs_solve_kernel / lbfgsb_solve_kernel: the production path) a segment that
finishes a constrained problem fetches the next one and must start clean: the multipliers in its LDS rows, the
auto-scaled penalty, the warm-up stopping test, the first evaluation the outer step reports against, the inner solver's
history and plateau ring.  With one problem per resident segment (every other auglag test but a sampled one) none of that
is exercised.  The batches are tests/alq_cases.py: problems of very different lengths back to back — penalties over five
decades, some auto-scaled, incoming multipliers, per-row term constants — and rows of NaN, +-inf and 1e100 spliced in.

Every capped case is checked three ways, every comparison bit for bit on x, lambda, mu, penalty, max_violation,
max_lagrangian_gradient and every field of the progress record (no tolerance anywhere in this file):
  1. capped device == the same solver on a fresh uncapped context, on every row, NaN payloads included;
  2. uncapped device == auglag_lib.oracle_minimize / oracle_box_minimize with reduction="butterfly" and the mapping's padded
     width — every row where n <= 64, every 4th row at n = 100 and every 2nd at n = 200 (18 rows each).  Against the CPU
     a NaN equals a NaN of another sign (the CPU's default NaN has the sign bit set, the GPU's not); every other bit, the
     sign of a zero included, must agree;
  3. not vacuous (_assert_refetches): the capped launch had exactly `cap` workgroups of the expected shape, the batch holds
     at least 4 x cap x (problem slots of a workgroup) rows and is no multiple of the segments of a wavefront, and the
     uncapped run's grid had a slot for every row, so the run that serves as the reference never fetched twice.  In the
     lock-step and auto loops the record is that of the LAST inner launch (one workgroup under cap 1); that the first
     launch of the uncapped run, the one with all rows, had a slot for each is read from a batch of NaN rows of the same
     size, which ends in its first outer iteration.

Cases (numbers of the issue that asked for them):
  1  fused, the mixed problem (every term kind and form) on the six mappings, caps 1 and 3
  2  fused, convergent batches (every row ends with status 6 after 2 to 18 outer iterations), n = 7 and 40
  3  fused over L-BFGS-B, n = 6, 12, 24, 48 (sixteen lanes, E = 1, 1, 2, 4) and 100 (the 32 x 4 kernel), bounds set (start
     coordinates on a bound) and never set, caps 1 and 2
  4  Hager-Zhang inner search, fused: n = 12 and 40 over Lbfgs, n = 12 over Lbfgsb
  5  a constraint family (auglag_launch_fused_family), cap 1
  6  lock-step under cap 1: n = 7 (36 outer iterations: chain-of-four launches, both half-rings of counters zeroed), n = 30,
     and n = 12 over Lbfgsb
  7  order independence: the n = 30 batch of case 1 and a seeded permutation of it under cap 1 permute bitwise
  8  loop = auto at n = 7: lock-step, then the hand-over of 215 survivors to the fused kernel after outer iteration 12,
     cap 1 and uncapped (the schedule is asserted from the oracle: alq_cases.check_handover_conditions)
  9  the device-tensor entry with term_constants on a capped context == minimize_host == the oracle, n = 40
  10 a user term: Hs029 on a context of libmi355_lbfgs_hs.so, fused and lock-step, cap 1
"""
import os

import numpy as np
import pytest

import alq_cases as A
import auglag_lib as al

pytestmark = pytest.mark.gpu


@pytest.fixture
def capped(monkeypatch, gpu_solver_factory):
    """capped(cap, library=None): a FRESH context created with the resident grid capped to `cap` workgroups (None: a
    fresh uncapped context).  (gpu_solver_factory is asked for first, so that the session's shared context can never be
    created while the variable is set.)"""
    import cppnumericalsolvers_amd as amd
    made = []

    def make(cap, library=None):
        if cap is None:
            monkeypatch.delenv(A.CAP_ENV, raising=False)
        else:
            monkeypatch.setenv(A.CAP_ENV, str(cap))
        ctx = amd.Context(0, library=library)
        monkeypatch.delenv(A.CAP_ENV, raising=False)
        made.append(ctx)
        return ctx

    yield make
    for ctx in made:
        ctx.close()


def _engine_problem(p):
    """The oracle's problem description as the engine's (user term functors go by their objective id)."""
    from cppnumericalsolvers_amd import ConstrainedProblem
    kind = lambda k: int(al.KIND[k]) if al.KIND[k] >= 100 else k
    mk = lambda t: ConstrainedProblem.term([(kind(q[0]),) + tuple(q[1:]) for q in t["prims"]], t["form"], t["k"],
                                           product=t.get("product", False))
    return ConstrainedProblem(p.n, mk(p.terms[0]), [mk(t) for t in p.table_eq], [mk(t) for t in p.table_ineq],
                              user_params=p.user_params, family_equality=p.family_equality,
                              family_inequality=p.family_inequality)


def _solver(ctx, case, loop=None):
    from cppnumericalsolvers_amd import BatchedAugmentedLagrangian, capi
    box = {} if case.lower is None else dict(lower=case.lower, upper=case.upper)
    s = BatchedAugmentedLagrangian(context=ctx, inner=case.inner, m=case.m, linesearch=case.linesearch, **box)
    cfg = case.config()
    for name, _ in cfg._fields_:
        setattr(s.config, name, getattr(cfg, name))
    s.config.loop = capi.AL_LOOP[loop or case.loop]
    if case.inner_iterations is not None:
        s.inner_stopping_progress.num_iterations = case.inner_iterations
    return s


def _none_if_empty(v):
    return None if v is None or v.shape[1] == 0 else v


def _run(solver, case, x0=None):
    """minimize_host on the case's state; (result, launch record)."""
    d = solver.minimize_host(_engine_problem(case.problem), case.x0 if x0 is None else x0,
                             lambda0=_none_if_empty(case.lambda0), mu0=_none_if_empty(case.mu0), penalty0=case.penalty0,
                             term_constants=case.term_constants)
    return d, solver.last_launch()


def _assert_shape(ll, case):
    assert (ll["lanes_per_problem"], ll["threads"]) == case.launch, (case.name, ll, case.launch)


def _assert_refetches(ll, cap, case):
    """The capped launch behind the record ll made every resident segment fetch four times or more on average."""
    _assert_shape(ll, case)
    per_wave, slots = A.segments(ll["lanes_per_problem"], ll["threads"])
    assert ll["blocks"] == cap, (case.name, ll, cap)                              # the cap reached this launch
    assert case.B >= 4 * cap * slots, (case.name, case.B, cap, slots)
    assert per_wave == 1 or case.B % per_wave != 0, (case.name, case.B, per_wave)  # a ragged last wavefront


def _assert_never_refetched(ll, rows, case):
    _assert_shape(ll, case)
    slots = A.segments(ll["lanes_per_problem"], ll["threads"])[1]
    assert ll["blocks"] * slots >= rows, (case.name, ll, rows)


def _assert_same_bits(a, b, what, slots=None, any_nan=False):
    diff = A.first_difference(a, b, slots=slots, any_nan=any_nan)
    assert diff is None, "%s: %s" % (what, diff)


def _assert_first_launch_never_refetched(ctx, case):
    """Lock-step and auto: the first inner launch takes all B rows, and the record that is left is a later launch's.  A
    batch of B rows of NaN ends in its first outer iteration, so its record is that first launch's."""
    s = _solver(ctx, case, loop="lockstep")
    d, ll = _run(s, case, x0=np.full_like(case.x0, np.nan))
    assert (d["progress"]["num_iterations"] == 1).all()
    _assert_never_refetched(ll, case.B, case)


_kept = {}   # results other tests compare with: {(case name, cap): result}


def _three_way(capped, case, library=None):
    """Uncapped device == the oracle; every capped run == the uncapped one, and refetches."""
    o = A.oracle(case)
    base, ll = _run(_solver(capped(None, library), case), case)
    if case.loop == "fused":
        _assert_never_refetched(ll, case.B, case)
    else:
        _assert_first_launch_never_refetched(capped(None, library), case)
    _assert_same_bits(A.take_rows(base, case.oracle_rows), o, "%s: uncapped device vs oracle" % case.name, any_nan=True)
    for cap in case.caps:
        out, ll = _run(_solver(capped(cap, library), case), case)
        _assert_refetches(ll, cap, case)
        _assert_same_bits(out, base, "%s: cap %d vs uncapped" % (case.name, cap), slots=cap * case.slots)
        _kept[(case.name, cap)] = out
    return base, o


# ---- 1, 2: the fused loop over Lbfgs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", A.FUSED_N)
def test_fused_mixed_problem_on_every_mapping(capped, n):
    """Case 1.  n = 200 runs the (64, 4) mapping: three wavefronts per workgroup, one problem each."""
    case = A.fused_mixed(n)
    A.check_batch(case)
    base, o = _three_way(capped, case)
    # the batch is what it is meant to be: rows stopped at once and rows stopped by the outer limit, back to back
    its, limit = base["progress"]["num_iterations"], case.cfg_kw["outer_num_iterations"]
    assert (its[case.spliced[[0, 2, 3]]] == 1).all() and np.sum(its == limit + 1) >= case.B // 2


@pytest.mark.parametrize("n", [7, 40])
def test_fused_convergent_batches(capped, n):
    """Case 2.  Every row converges (status 6), after numbers of outer iterations that differ by 8 or more."""
    case = A.fused_convergent(n)
    A.check_batch(case)
    base, o = _three_way(capped, case)
    its = o["progress"]["num_iterations"]
    assert (o["progress"]["status"] == 6).all() and its.max() >= its.min() + 8, (its.min(), its.max())


# ---- 3, 4: L-BFGS-B inside, Hager-Zhang ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", ["set", "never_set"])
@pytest.mark.parametrize("n", A.BOX_N)
def test_fused_over_lbfgsb(capped, n, bounds):
    """Case 3.  Caps 1 and 2.

    With the bounds set these batches also pin what the L-BFGS-B kernel does on a NaN gradient (the rows with a NaN or
    infinite start coordinate): every breakpoint is then a NaN, the reference's sort leaves the coordinates in index
    order, its Cauchy point drifts the last of them, n - 1, by a NaN step, and the returned x holds a NaN there even
    where the start sat on a bound.  (The kernel used to leave that coordinate on its bound: uncapped device != oracle
    in x[n - 1] of those rows at n = 12, 48 and 100.)"""
    case = A.fused_box(n, bounds)
    A.check_batch(case)
    base, o = _three_way(capped, case)
    if bounds == "set":
        ok = ~np.isnan(base["x"])
        assert ((base["x"] >= case.lower) | ~ok).all() and ((base["x"] <= case.upper) | ~ok).all()
        assert ((case.x0 == case.lower) | (case.x0 == case.upper)).any(axis=1).sum() >= 4      # starts on a bound


@pytest.mark.parametrize("inner,n", [("lbfgs", 12), ("lbfgs", 40), ("lbfgsb", 12)])
def test_fused_with_the_hager_zhang_search(capped, inner, n):
    """Case 4."""
    case = A.fused_hager_zhang(n) if inner == "lbfgs" else A.fused_box(n, "set", "hager_zhang", caps=(1, 3))
    A.check_batch(case)
    _three_way(capped, case)


# ---- 5: a constraint family ------------------------------------------------------------------------------------------------
def test_fused_family(capped):
    """Case 5: table terms ahead of 8 family equalities and 24 family inequalities, n = 16."""
    case = A.fused_family()
    A.check_batch(case)
    assert case.problem.family_equality is not None and case.problem.family_inequality is not None
    assert len(case.problem.table_eq) == 1 and len(case.problem.table_ineq) == 1
    _three_way(capped, case)


# ---- 6: lock-step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner,n", sorted(A.LOCKSTEP))
def test_lockstep_on_one_workgroup(capped, inner, n):
    """Case 6.  Every inner launch after the first goes through problem_map and count_dev; past outer iteration 4 they
    come four to a read-back, bounded by the last count read; at n = 7 the loop passes iteration 32, where the second
    half of the counter ring is zeroed."""
    case = A.lockstep(inner, n)
    A.check_batch(case)
    its = A.oracle(case)["progress"]["num_iterations"]
    assert A.survivors(its, 8) > 0
    if case.cfg_kw["outer_num_iterations"] > 32:
        assert A.survivors(its, 32) > 0
    _three_way(capped, case)


# ---- 7: order independence -------------------------------------------------------------------------------------------------
def test_fused_results_do_not_depend_on_the_order_of_the_batch(capped):
    """Case 7.  Needs no oracle: the same rows in another queue order, on one workgroup."""
    case = A.fused_mixed(30)
    perm = np.random.default_rng(A.SEED + 30).permutation(case.B)
    assert (perm != np.arange(case.B)).mean() > 0.9
    if (case.name, 1) not in _kept:
        out, ll = _run(_solver(capped(1), case), case)
        _assert_refetches(ll, 1, case)
        _kept[(case.name, 1)] = out
    shuffled = case.permuted(perm)
    out, ll = _run(_solver(capped(1), shuffled), shuffled)
    _assert_refetches(ll, 1, shuffled)
    _assert_same_bits(out, A.take_rows(_kept[(case.name, 1)], perm), "%s permuted" % case.name, slots=case.slots)


# ---- 8: auto, the hand-over ------------------------------------------------------------------------------------------------
def test_auto_hands_the_survivors_to_the_fused_kernel_in_the_chain_of_four_regime(capped):
    """Case 8.  The fused launch of the hand-over goes through the map of the lock-step loop and begins problems whose
    first outer iteration is long past; under cap 1 its one workgroup fetches the handed-over rows three times over."""
    case = A.handover()
    A.check_batch(case)
    o = A.oracle(case)
    schedule, r = A.check_handover_conditions(case, o)
    handed = schedule[-1][1]
    print("survivors at the read-backs: %s" % ", ".join("rem(%d) = %d" % s for s in schedule))
    base, ll = _run(_solver(capped(None), case), case)
    _assert_never_refetched(ll, handed, case)        # the record is the hand-over launch's: a slot for every survivor
    # ... and exactly the workgroups those survivors need (a lock-step loop that went on to the end would leave the record
    # of a launch bounded by the far smaller count of a later read-back)
    assert ll["blocks"] == -(-handed // case.slots) and A.survivors(o["progress"]["num_iterations"], r + 4) <= handed // 2
    _assert_first_launch_never_refetched(capped(None), case)
    _assert_same_bits(base, o, "%s: uncapped device vs oracle" % case.name, any_nan=True)
    out, ll = _run(_solver(capped(1), case), case)
    _assert_refetches(ll, 1, case)
    assert handed >= 3 * A.segments(ll["lanes_per_problem"], ll["threads"])[1]
    _assert_same_bits(out, base, "%s: cap 1 vs uncapped" % case.name)
    # the two pure forms of the loop agree with it (one workgroup each)
    for loop in ("fused", "lockstep"):
        other, ll = _run(_solver(capped(1), case, loop=loop), case)
        _assert_refetches(ll, 1, case)
        _assert_same_bits(other, base, "%s: loop=%s under cap 1 vs auto uncapped" % (case.name, loop))


# ---- 9: the device-tensor entry --------------------------------------------------------------------------------------------
def test_device_tensor_entry_under_a_cap(capped):
    """Case 9.  minimize (device tensors, asynchronous) with term_constants on a capped context == minimize_host on an
    uncapped one == the oracle."""
    import torch
    from cppnumericalsolvers_amd import capi
    case = A.device_entry()
    A.check_batch(case)
    base, o = _three_way(capped, case)
    s = _solver(capped(1), case)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x, lam, mu, pen, tc = up(case.x0), up(case.lambda0), up(case.mu0), up(case.penalty0), up(case.term_constants)
    viol, kkt, prog = s.minimize(_engine_problem(case.problem), x, lam, mu, pen, term_constants=tc)
    torch.cuda.synchronize()
    _assert_refetches(s.last_launch(), 1, case)
    got = {"x": x.cpu().numpy(), "lambda": lam.cpu().numpy(), "mu": mu.cpu().numpy(), "penalty": pen.cpu().numpy(),
           "max_violation": viol.cpu().numpy(), "max_lagrangian_gradient": kkt.cpu().numpy(),
           "progress": prog.cpu().numpy().view(capi.AL_PROGRESS_DTYPE)}
    _assert_same_bits(got, base, "%s: device entry under cap 1 vs host entry uncapped" % case.name, slots=case.slots)


# ---- 10: a user term -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", ["fused", "lockstep"])
def test_user_terms_under_a_cap(capped, loop):
    """Case 10.  Hs029 (user objective and user constraint) in the library built with the Hock-Schittkowski functors."""
    from cppnumericalsolvers_amd import _build
    path = os.path.join(_build.PKG_DIR, "libmi355_lbfgs_hs.so")
    assert os.path.exists(path), "the example library is built by __graft_entry__.build() and travels with the tree"
    case = A.user_terms(loop)
    A.check_batch(case)
    _three_way(capped, case, library=path)
