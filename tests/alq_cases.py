"""Case builders of the augmented-Lagrangian work-queue tests (tests/test_gpu_auglag_queue.py on the device,
tests/test_auglag_queue_cases.py on the CPU oracle): mixed batches that give a persistent kernel constrained problems of
very different lengths back to back, with degenerate rows spliced in, sized so that a grid capped to a few workgroups
fetches every segment at least four times.

A case is a `Case`: the problem, the per-row state (x0, multipliers, penalty0, term constants), the solver's options and
the launch the library is expected to pick for it, (lanes per problem, threads of a workgroup) — the batch size follows
from those, and the device test asserts the launch record against them.  Nothing here touches the GPU."""
import numpy as np

import auglag_lib as al

SEED = 20261020
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"

STATE_FIELDS = ("x", "lambda", "mu", "penalty", "max_violation", "max_lagrangian_gradient")
PROGRESS_FIELDS = ("status", "num_iterations", "x_delta", "f_delta", "gradient_norm", "inner_iterations", "nfev", "sum_k")

# The launch of the Lbfgs inner solver on the composite objective at its default m = 10 (csrc/engine_internal.hpp
# launch_solve): n -> (lanes per problem, threads of a workgroup).  The wavefronts of a workgroup share the term table in
# LDS; as many as fit next to it, at most 8 (4 on the (64, 4) mapping).
LBFGS_LAUNCH = {7: (8, 512), 12: (8, 384), 30: (16, 384), 40: (32, 448), 64: (32, 448), 100: (64, 384), 200: (64, 192)}
# ... with a constraint family of 4 x lanes rows next to each problem's history (csrc/auglag_family.hip), n = 16
FAMILY_LAUNCH = {16: (8, 256)}
# The Lbfgsb inner solver: one wavefront per workgroup, sixteen lanes per problem (thirty-two for 64 < n <= 128)
LBFGSB_LAUNCH = {6: (16, 64), 12: (16, 64), 24: (16, 64), 48: (16, 64), 100: (32, 64)}


def padded(n):
    P = 8
    while P < n:
        P <<= 1
    return P


def segments(lanes, threads):
    """(segments of a wavefront, problem slots of a workgroup)"""
    return 64 // lanes, (64 // lanes) * (threads // 64)


def smallest_batch(launch, max_cap):
    """The smallest B with B >= 4 x max_cap x (slots of a workgroup) that is no multiple of the segments of a wavefront
    (where a wavefront holds more than one)."""
    per_wave, slots = segments(*launch)
    B = 4 * max_cap * slots
    return B + 1 if per_wave > 1 else B


def spliced_positions(B):
    """Six rows spread over the batch, the first and the last among them, never two of them neighbours: every degenerate
    row but the last is followed by an ordinary one."""
    pos = sorted({0, B // 6 + 1, (2 * B) // 6, (3 * B) // 6 + 1, (4 * B) // 6, B - 1})
    assert len(pos) == 6 and min(np.diff(pos)) >= 2, pos
    return np.array(pos)


def splice(x0, rng):
    """Degenerate starts at spliced_positions: a row of NaN, one NaN coordinate, one +inf, one -inf, a row of 1e100, one
    1e100 coordinate."""
    B, n = x0.shape
    pos = spliced_positions(B)
    col = rng.integers(0, n, size=6)
    x0[pos[0], :] = np.nan
    x0[pos[1], col[1]] = np.nan
    x0[pos[2], col[2]] = np.inf
    x0[pos[3], col[3]] = -np.inf
    x0[pos[4], :] = 1e100
    x0[pos[5], col[5]] = 1e100
    return pos


class Case:
    def __init__(self, name, problem, x0, launch, caps, cfg_kw, lambda0=None, mu0=None, penalty0=0.0, term_constants=None,
                 inner="lbfgs", m=None, linesearch="more_thuente", lower=None, upper=None, loop="fused", spliced=(),
                 oracle_stride=1, inner_iterations=None):
        self.name, self.problem, self.x0, self.launch, self.caps = name, problem, x0, launch, tuple(caps)
        self.cfg_kw, self.lambda0, self.mu0, self.term_constants = dict(cfg_kw), lambda0, mu0, term_constants
        self.penalty0 = np.broadcast_to(np.asarray(penalty0, dtype=np.float64), (x0.shape[0],)).copy()
        self.inner, self.linesearch, self.lower, self.upper, self.loop = inner, linesearch, lower, upper, loop
        self.m = (5 if inner == "lbfgsb" else 10) if m is None else m
        self.spliced = np.asarray(spliced, dtype=int)
        # num_iterations of the inner solver's stopping test (None: its default, 10000)
        self.inner_iterations = inner_iterations
        # rows the oracle is asked for: every row where n <= 64, every oracle_stride-th above
        self.oracle_stride = oracle_stride
        assert oracle_stride == 1 or problem.n > 64

    @property
    def B(self):
        return self.x0.shape[0]

    @property
    def n(self):
        return self.problem.n

    @property
    def slots(self):
        return segments(*self.launch)[1]

    @property
    def oracle_rows(self):
        return np.arange(0, self.B, self.oracle_stride)

    def config(self):
        return al.default_config(**self.cfg_kw)

    def inner_stop(self):
        """The inner solver's stopping record, as the oracle takes it."""
        import oracle_lib
        st = oracle_lib.lbfgsb_default_stop() if self.inner == "lbfgsb" else oracle_lib.default_stop()
        if self.inner_iterations is not None:
            st.num_iterations = self.inner_iterations
        return st

    def rows(self, idx):
        """The inputs of the rows idx, as keyword arguments of the oracle calls."""
        sub = lambda v: None if v is None else v[idx]
        return dict(x0=self.x0[idx], lambda0=sub(self.lambda0), mu0=sub(self.mu0), penalty0=self.penalty0[idx],
                    term_constants=sub(self.term_constants))

    def permuted(self, perm):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        sub = lambda v: None if v is None else v[perm]
        c.x0, c.lambda0, c.mu0, c.penalty0, c.term_constants = (self.x0[perm], sub(self.lambda0), sub(self.mu0),
                                                                self.penalty0[perm], sub(self.term_constants))
        return c


_oracle_cache = {}


def oracle(case, idx=None):
    """The CPU oracle in the device's summation order on the rows idx (default: case.oracle_rows), computed once per case
    and left unchanged."""
    key = (case.name, None if idx is None else tuple(idx))
    if key not in _oracle_cache:
        kw = case.rows(case.oracle_rows if idx is None else idx)
        x0 = kw.pop("x0")
        common = dict(config=case.config(), inner_stop=case.inner_stop(), m=case.m, linesearch=case.linesearch,
                      reduction="butterfly", width=padded(case.n), **kw)
        if case.inner == "lbfgsb":
            box = {} if case.lower is None else dict(lower=case.lower, upper=case.upper)
            out = al.oracle_box_minimize(case.problem, x0, std_sort_order=False, **box, **common)
        else:
            out = al.oracle_minimize(case.problem, x0, **common)
        for v in out.values():
            v.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1) if a.size else np.zeros((a.shape[0], 0), dtype=np.uint8)


def _columns(d):
    for k in STATE_FIELDS:
        yield k, d[k]
    for k in PROGRESS_FIELDS:
        yield "progress." + k, d["progress"][k]


def first_difference(a, b, slots=None, any_nan=False):
    """None when every compared field of the results a and b holds the same bits, else a description: the field, how
    many rows differ and the first of them.  In the fused loop a row's index is its position in the queue: with `slots`
    problem slots resident, rows >= slots were fetched by a segment that had solved another problem before.
    any_nan: a NaN equals a NaN of another sign or payload (the CPU's default NaN has the sign bit set, the GPU's has
    not); everything else, the sign of a zero included, is compared bit for bit."""
    for (name, u), (_, v) in zip(_columns(a), _columns(b)):
        if u.shape != v.shape:
            return "%s: shapes %s and %s" % (name, u.shape, v.shape)
        if u.size == 0:
            continue
        diff = _bits(u) != _bits(v)
        if any_nan and u.dtype.kind == "f":
            both = (np.isnan(u) & np.isnan(v)).reshape(u.shape[0], -1)
            diff = diff.reshape(u.shape[0], both.shape[1], -1).any(axis=2) & ~both
        rows = np.nonzero(diff.reshape(u.shape[0], -1).any(axis=1))[0]
        if rows.size:
            where = "" if slots is None else " (queue positions; %d resident slots per workgroup)" % slots
            r = rows[0]
            return "%s differs in %d of %d rows, first rows %s%s: %r != %r" % (name, rows.size, u.shape[0], rows[:8].tolist(),
                                                                           where, u[r], v[r])
    return None


def take_rows(d, idx):
    out = {k: d[k][idx] for k in STATE_FIELDS}
    out["progress"] = d["progress"][idx]
    return out


# ---- the batches ---------------------------------------------------------------------------------------------------------
def _constants(problem, B, rng):
    """Per-row constants k of the terms: each of the problem's own, scaled by U(0.8, 1.2) (a constant of 0 stays 0)."""
    return np.ascontiguousarray(problem.ks[None, :] * rng.uniform(0.8, 1.2, (B, len(problem.terms))))


def mixed_state(problem, B, rng, x_scale=1.5, constants=True, decades=(-3.0, 2.0)):
    """Random starts; penalty0 spread over several decades (every fifth row 0: the penalty is auto-scaled on the device
    when the configuration asks for it), so long problems follow short ones; non-zero incoming multipliers on every second
    row; per-row term constants; degenerate rows spliced in.  Returns the keyword arguments of Case."""
    n = problem.n
    x0 = rng.uniform(-x_scale, x_scale, (B, n))
    pos = splice(x0, rng)
    pen = 10.0 ** rng.uniform(decades[0], decades[1], B)
    pen[4::5] = 0.0
    lam = rng.uniform(-1.0, 1.0, (B, problem.n_eq))
    mu = rng.uniform(0.0, 2.0, (B, problem.n_ineq))
    lam[1::2] = 0.0
    mu[1::2] = 0.0
    return dict(x0=x0, lambda0=lam, mu0=mu, penalty0=pen, spliced=pos,
                term_constants=_constants(problem, B, rng) if constants else None)


def mixed_problem(n, seed):
    """tests/test_gpu_auglag.py _mixed_problem: every term kind and form, two equalities, two inequalities."""
    rng = np.random.default_rng(seed)
    return al.Problem(
        n, al.term("rosenbrock"),
        [al.term("linear", "value_minus_k", 0.3, a=rng.uniform(-1, 1, n)),
         al.term("diag_quadratic", "k_minus_value", 2.0, a=rng.uniform(0.1, 1.0, n), c=0.25)],
        [al.term("squared_norm", "k_minus_value", 0.4 * n),
         al.term("linear", "plain", a=rng.uniform(0.0, 1.0, n))])


FUSED_N = (7, 12, 30, 64, 100, 200)            # the six mappings (8,1) (8,2) (16,2) (32,2) (64,2) (64,4)
FUSED_OUTER_LIMIT = {7: 15, 12: 15, 30: 12, 64: 8, 100: 6, 200: 4}
# n > 64: the oracle solves every ORACLE_STRIDE-th row (18 rows each); capped == uncapped is compared on every row
ORACLE_STRIDE = {100: 4, 200: 2}


def fused_mixed(n):
    """Case 1: the fused loop on the mixed problem, one case per mapping."""
    caps = (1, 3)
    launch = LBFGS_LAUNCH[n]
    p = mixed_problem(n, seed=n)
    rng = np.random.default_rng(SEED + n)
    return Case("fused_mixed_%d" % n, p, launch=launch, caps=caps, cfg_kw=dict(outer_num_iterations=FUSED_OUTER_LIMIT[n]),
                oracle_stride=ORACLE_STRIDE.get(n, 1), **mixed_state(p, smallest_batch(launch, max(caps)), rng))


CONVERGENT_CONFIG = dict(auto_scale_initial_penalty=0, penalty_growth_factor=4.0, warmup_max_inner_iterations=0,
                         outer_num_iterations=30)


def convergent_state(n, B, rng):
    """The recipe of the hand-over case: starts in [-2, 2], penalty0 = 10 ** U(-6, 2) per row, no auto-scaling, growth
    factor 4: every row converges, the small penalties after many outer iterations, the large ones after few."""
    return dict(x0=rng.uniform(-2.0, 2.0, (B, n)), penalty0=10.0 ** rng.uniform(-6.0, 2.0, B))


def fused_convergent(n):
    """Case 2: every row ends with status 6 after very different numbers of outer iterations."""
    caps = (1, 3)
    launch = LBFGS_LAUNCH[n]
    rng = np.random.default_rng(SEED + 100 + n)
    return Case("fused_convergent_%d" % n, al.quadratic_simplex_problem(n, seed=5), launch=launch, caps=caps,
                cfg_kw=CONVERGENT_CONFIG, **convergent_state(n, smallest_batch(launch, max(caps)), rng))


BOX_N = (6, 12, 24, 48, 100)                   # E = 1, 1, 2, 4 on sixteen lanes, then the 32 x 4 kernel
# num_iterations of the inner Lbfgsb: now and then an ordinary row stalls and runs every inner solve into its limit — a
# row the queue tests want (a long problem among short ones), at a length (the default is 10000) that keeps a case short
BOX_INNER_LIMIT = 500


def _put_on_bounds(x0, lower, upper, spliced):
    """Some start coordinates on a bound exactly, one ordinary row in a corner of the box."""
    keep = x0[spliced].copy()
    x0[1::4, ::2] = lower[::2]
    x0[2::5, 1::2] = upper[1::2]
    corner = x0.shape[0] // 2
    x0[corner] = upper
    x0[spliced] = keep
    return corner


def fused_box(n, bounds, linesearch="more_thuente", caps=(1, 2)):
    """Cases 3 and 4: the fused loop around the L-BFGS-B kernel; bounds "set" (start coordinates on a bound) or
    "never_set"."""
    launch = LBFGSB_LAUNCH[n]
    p, lower, upper = al.boxed_rosenbrock_problem(n)
    rng = np.random.default_rng(SEED + 200 + n + (1 if bounds == "set" else 0))
    st = mixed_state(p, smallest_batch(launch, max(caps)), rng, x_scale=1.0)
    box = {}
    if bounds == "set":
        _put_on_bounds(st["x0"], lower, upper, st["spliced"])
        box = dict(lower=lower, upper=upper)
    hz = linesearch == "hager_zhang"
    return Case("fused_box_%d_%s%s" % (n, bounds, "_hz" if hz else ""), p, launch=launch, caps=caps,
                cfg_kw=dict(outer_num_iterations=10), inner="lbfgsb", m=3 if hz else 5, linesearch=linesearch,
                inner_iterations=BOX_INNER_LIMIT, **box, **st)


def fused_hager_zhang(n):
    """Case 4 over Lbfgs: the mixed state on the convex problem of the neighbouring Hager-Zhang test."""
    caps = (1, 3)
    launch = LBFGS_LAUNCH[n]
    p = al.quadratic_simplex_problem(n, seed=n)
    rng = np.random.default_rng(SEED + 300 + n)
    return Case("fused_hz_%d" % n, p, launch=launch, caps=caps, cfg_kw=dict(outer_num_iterations=25),
                linesearch="hager_zhang", **mixed_state(p, smallest_batch(launch, max(caps)), rng, x_scale=1.0))


FAMILY_SHAPE = (16, 8, 24, True)               # of tests/test_gpu_auglag_family.py SHAPES: table terms and both families


def fused_family():
    """Case 5: auglag_launch_fused_family.  (The entry takes no per-row constants next to a family.)"""
    n, f_eq, f_ineq, table = FAMILY_SHAPE
    caps = (1,)
    launch = FAMILY_LAUNCH[n]
    p = al.random_family_problem(n, f_eq, f_ineq, seed=n, table=table)
    rng = np.random.default_rng(SEED + 400 + n)
    return Case("fused_family_%d" % n, p, launch=launch, caps=caps, cfg_kw=dict(outer_num_iterations=15),
                **mixed_state(p, smallest_batch(launch, max(caps)), rng, x_scale=1.0, constants=False))


# outer_num_iterations of the lock-step cases: past 8 the chain-of-four launches run, past 32 the second half of the ring
# of per-iteration counters is zeroed while the first is still being read (csrc/auglag.hip)
LOCKSTEP = {("lbfgs", 7): 36, ("lbfgs", 30): 12, ("lbfgsb", 12): 12}


def lockstep(inner, n):
    """Case 6: the lock-step loop on one workgroup — inner launches through problem_map / count_dev."""
    caps = (1,)
    limit = LOCKSTEP[(inner, n)]
    rng = np.random.default_rng(SEED + 500 + n)
    if inner == "lbfgsb":
        launch = LBFGSB_LAUNCH[n]
        p, lower, upper = al.boxed_rosenbrock_problem(n)
        st = mixed_state(p, smallest_batch(launch, 1), rng, x_scale=1.0)
        _put_on_bounds(st["x0"], lower, upper, st["spliced"])
        return Case("lockstep_box_%d" % n, p, launch=launch, caps=caps, cfg_kw=dict(outer_num_iterations=limit),
                    inner="lbfgsb", lower=lower, upper=upper, loop="lockstep", inner_iterations=BOX_INNER_LIMIT, **st)
    launch = LBFGS_LAUNCH[n]
    p = mixed_problem(n, seed=n)
    return Case("lockstep_%d" % n, p, launch=launch, caps=caps, cfg_kw=dict(outer_num_iterations=limit), loop="lockstep",
                **mixed_state(p, smallest_batch(launch, 1), rng))


def survivors(num_iterations, r):
    """rem(r): rows that continue past outer iteration r (finished rows report the iteration they stopped in; a row
    stopped by the limit L reports L + 1)."""
    return int(np.sum(np.asarray(num_iterations) > r))


HANDOVER_B = 700
HANDOVER_TAIL = 256                            # kFusedTail of csrc/auglag.hip
HANDOVER_SEED = SEED + 600


def handover():
    """Case 8: loop = auto at eight lanes per problem — lock-step, then the survivors to the fused kernel in mid-run."""
    n, B = 7, HANDOVER_B
    rng = np.random.default_rng(HANDOVER_SEED)
    return Case("handover_7", al.quadratic_simplex_problem(n, seed=5), launch=LBFGS_LAUNCH[n], caps=(1,),
                cfg_kw=CONVERGENT_CONFIG, loop="auto", **convergent_state(n, B, rng))


def handover_schedule(num_iterations):
    """The read-backs of the lock-step driver (after outer iterations 1, 2, 3, 4, 8, 12, ...) with the survivors each one
    sees, up to the one that hands over (0 < survivors <= 256) or ends the loop: [(r, rem(r)), ...]."""
    out = []
    r = 0
    while True:
        r += 1 if r < 4 else 4
        rem = survivors(num_iterations, r)
        out.append((r, rem))
        if rem <= HANDOVER_TAIL:
            return out


def check_handover_conditions(case, o):
    """The input conditions of case 8 on the oracle's result o; returns (the schedule, r of the hand-over)."""
    its, limit = o["progress"]["num_iterations"], case.cfg_kw["outer_num_iterations"]
    schedule = handover_schedule(its)
    r, rem = schedule[-1]
    assert survivors(its, 4) > HANDOVER_TAIL, schedule                       # the chain-of-four regime is reached
    assert r >= 8 and r % 4 == 0 and 0 < rem <= HANDOVER_TAIL, schedule       # ... and the hand-over happens in it
    assert all(m > HANDOVER_TAIL for _, m in schedule[:-1]), schedule        # (the first such read-back)
    assert rem >= 3 * case.slots, (schedule, case.slots)                      # the handed-over rows refetch on one workgroup
    assert (o["progress"]["status"] == 6).all() and its.max() <= limit       # no row ends on the iteration limit
    return schedule, r


def device_entry():
    """Case 9: the device-tensor entry with per-row constants, n = 40."""
    n, caps = 40, (1,)
    launch = LBFGS_LAUNCH[n]
    p = al.quadratic_simplex_problem(n, seed=21)
    rng = np.random.default_rng(SEED + 700)
    return Case("device_entry_40", p, launch=launch, caps=caps, cfg_kw=dict(outer_num_iterations=15),
                **mixed_state(p, smallest_batch(launch, 1), rng, x_scale=1.0))


USER_LAUNCH = (8, 512)                         # n = 2 in the library of the Hock-Schittkowski term functors


def user_terms(loop):
    """Case 10: Hs029 — user objective and user constraint — fused and lock-step."""
    rng = np.random.default_rng(SEED + 800)
    B = smallest_batch(USER_LAUNCH, 1)
    x0 = np.vstack([[1.0, 1.0], rng.uniform(0.3, 3.0, (B - 61, 2)), rng.uniform(-3.0, 3.0, (60, 2))])
    pos = splice(x0, rng)
    pen = 10.0 ** rng.uniform(-3.0, 2.0, B)
    pen[4::5] = 0.0
    return Case("user_hs029_%s" % loop, al.hs029_problem(), x0, launch=USER_LAUNCH, caps=(1,),
                cfg_kw=dict(outer_num_iterations=30), penalty0=pen, loop=loop, spliced=pos)


def check_batch(case, max_cap=None):
    """What makes a capped run of the case non-vacuous, as far as the inputs decide it."""
    per_wave, slots = segments(*case.launch)
    cap = max(case.caps) if max_cap is None else max_cap
    assert case.B >= 4 * cap * slots, (case.name, case.B, cap, slots)
    assert per_wave == 1 or case.B % per_wave != 0, (case.name, case.B, per_wave)
    if case.spliced.size:
        assert min(np.diff(case.spliced)) >= 2 and not np.isfinite(case.x0[case.spliced[:4]]).all(axis=1).any()
        assert (case.x0[case.spliced[4:]] == 1e100).any(axis=1).all()
        ordinary = np.setdiff1d(np.arange(case.B), case.spliced)
        assert np.isfinite(case.x0[ordinary]).all()
        assert np.isin(case.spliced[:-1] + 1, ordinary).all()                # each followed by an ordinary row
    pen = case.penalty0[case.penalty0 > 0]
    assert pen.max() / pen.min() >= 1e3, (case.name, pen.min(), pen.max())    # spread over several decades
