"""The peeled More-Thuente search of the lean solve kernels (mt_cvsrch_peeled, csrc/more_thuente_device.hpp) at its corners.

The lean kernels run the first trial of every line search as straight-line code with brackt = false, stx = 0, nfev = 0 and
infoc = 1 folded in, and enter the general loop only for the segments whose first trial decided nothing.  No fp64
operation moves, so the results must be the BITS of the CPU twin (oracle, fused butterfly order) and of the general
kernel.  The flagship batches hardly leave the common path (first trial accepted, or one more trial), so this module
builds a batch that does, and proves on the CPU — before anything runs on the device — that each corner is reached:

  q1         g = 0 (the start of exact ones), or g.g overflowing: the fallback direction gives dginit >= 0 and the search
             returns at once without an evaluation (quirk Q1): nfev stays 1.
  stpmin     ||g0|| > 1e15, so the first iteration's initial step 1 / ||g0|| is clamped to stpmin = 1e-15, f finite
             there, and the search ends at that first trial (one evaluation in iteration 1).
  nonfinite  the same clamp, but f is not finite at the first trial: one evaluation, the solver restores the start
             state and stops on x_delta after one iteration with nfev = 2.
  maxfev     a line search that uses all 20 evaluations (trial values overflow until the step has shrunk).
  ordinary   the synthetic flagship starts and starts next to the minimiser: solves of very different lengths, so that
             under a capped grid a freshly fetched problem (k < m stored pairs) iterates beside old ones (k = m) in one
             wavefront; the batch is ragged (not a multiple of the segments of a wavefront).

The per-iteration evaluation counts come from the twin alone: nfev under the iteration limits L and L + 1 differ by the
evaluations of one line search.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CAP_ENV = "MI355_DEBUG_SOLVE_BLOCKS"
FIELDS = ("status", "num_iterations", "nfev", "sum_k", "x_delta", "f_delta", "gradient_norm")
MAXFEV = 20
STPMIN = 1e-15


def _twin(oracle, x0, m, E, limit=None):
    stop = oracle.parity_stop()
    if limit is not None:
        stop.num_iterations = limit
    return oracle.minimize_batch("rosenbrock", x0, m=m, stop=stop, reduction="butterfly_fma", width=x0.shape[1], fma_group=E)


def _sequences(oracle, x0, m, E, depth=14):
    """seq[b][i] = objective evaluations of the line search of iteration i + 1 of row b, for the iterations that ran
    (None where the twin's totals cannot separate it).  Iteration 1 alone: x_delta = 1e300 stops every solve with a
    finite step after its first iteration.  Later ones: the limit test is num_iterations > limit, so limit L stops
    after iteration L + 1, and nfev under L and L - 1 differ by the evaluations of iteration L + 1."""
    stop = oracle.parity_stop()
    stop.x_delta, stop.num_iterations = 1e300, 1
    p = oracle.minimize_batch("rosenbrock", x0, m=m, stop=stop, reduction="butterfly_fma", width=x0.shape[1], fma_group=E)[3]
    first = [int(p["nfev"][b]) - 1 if p["num_iterations"][b] == 1 else None for b in range(len(x0))]
    totals, its = [np.ones(len(x0), dtype=np.int64)], [np.zeros(len(x0), dtype=np.int64)]
    for limit in range(1, depth):
        p = _twin(oracle, x0, m, E, limit=limit)[3]
        totals.append(p["nfev"].astype(np.int64))
        its.append(p["num_iterations"].astype(np.int64))
    seqs = []
    for b in range(len(x0)):
        seq = [first[b]]
        if its[1][b] == 2:                                  # iteration 2 ran
            seq.append(int(totals[1][b]) - 1 - first[b] if first[b] is not None else None)
        for L in range(2, depth):
            if its[L][b] == L + 1 and its[L - 1][b] == L:   # iteration L + 1 ran
                seq.append(int(totals[L][b] - totals[L - 1][b]))
        seqs.append(seq)
    return seqs


def corner_batch(oracle, n, seed=20261017):
    """(x0, classes): the batch described in the module docstring, rows of the classes interleaved."""
    import cppnumericalsolvers_amd as amd
    rng = np.random.default_rng(seed + n)
    rows, cls = [], []

    def add(name, x):
        rows.append(np.asarray(x, dtype=np.float64))
        cls.append(name)

    std = amd.synthetic_x0_host(96, n, "std", seed=seed)
    u2 = amd.synthetic_x0_host(96, n, "u2", seed=seed)
    for i in range(96):
        add("ordinary", std[i] if i % 2 == 0 else u2[i])
        if i % 3 == 0:
            add("ordinary", 1.0 + 0.05 * rng.uniform(-1, 1, n))
        if i % 8 == 1:
            add("q1", np.ones(n))
        if i % 8 == 2:
            x = np.ones(n)
            x[i % n if i % n != n - 1 else 0] = 3e76       # f finite, g.g = inf
            add("q1", x)
        if i % 8 == 3:
            add("stpmin", 1e6 * rng.uniform(-1, 1, n))
        if i % 8 == 4:
            x = np.ones(n)
            x[(i * 7) % (n - 1)] = 1e38 if i % 16 == 4 else -1e38
            add("nonfinite", x)
        if i % 8 == 5:
            add("maxfev", 1e20 * rng.uniform(-1, 1, n))
        if i % 8 == 6:
            x = np.ones(n)
            x[n - 1] = -(10.0 ** rng.integers(38, 51))
            add("maxfev", x)
    while len(rows) % 8 != 3:                               # ragged for 8 and for 4 segments per wavefront
        add("ordinary", 1.0 + 1e-3 * rng.uniform(-1, 1, n))
    x0 = np.array(rows)
    return x0, np.array(cls)


def prove_corners(oracle, x0, cls, m, E):
    """Every class does on the CPU twin what the module docstring says (no device involved)."""
    x, f, g, p = _twin(oracle, x0, m, E)
    seqs = _sequences(oracle, x0, m, E)
    f0 = np.empty(len(x0))
    g0 = np.empty_like(x0)
    for b, row in enumerate(x0):
        f0[b], g0[b] = oracle.evaluate("rosenbrock", row, reduction="butterfly_fma", width=x0.shape[1], fma_group=E)
    assert np.all(np.isfinite(f0)), "every start has a finite value"
    count = {}
    for b in range(len(x0)):
        c = cls[b]
        count[c] = count.get(c, 0) + 1
        if c == "q1":
            gg = float(np.dot(g0[b], g0[b]))
            assert gg == 0.0 or np.isinf(gg), (b, gg)
            assert p["nfev"][b] == 1 and p["num_iterations"][b] >= 1, (b, p[b])
        elif c in ("stpmin", "nonfinite"):
            norm = float(np.sqrt(np.dot(g0[b], g0[b])))
            assert np.isfinite(norm) and 1.0 / norm < STPMIN, (b, norm)      # the initial step is clamped to stpmin
            trial = oracle.evaluate("rosenbrock", x0[b] - STPMIN * g0[b], reduction="butterfly_fma", width=x0.shape[1],
                                    fma_group=E)[0]
            if c == "stpmin":
                assert np.isfinite(trial), (b, trial)
                assert seqs[b][0] == 1, (b, seqs[b])      # iteration 1: the search ended at the clamped first trial
            else:
                assert not np.isfinite(trial), (b, trial)
                assert p["nfev"][b] == 2 and p["num_iterations"][b] == 1 and p["status"][b] == 2, (b, p[b])
        elif c == "maxfev":
            assert MAXFEV in seqs[b], (b, seqs[b])
        else:
            assert np.isfinite(f[b]) and p["status"][b] >= 2, (b, p[b])
    for c in ("ordinary", "q1", "stpmin", "nonfinite", "maxfev"):
        assert count.get(c, 0) >= 8, count
    it = p["num_iterations"][cls == "ordinary"]
    assert it.max() >= 4 * it.min() and it.min() > 10, (it.min(), it.max())   # short solves next to long ones, all past k = m
    # second and later trials are common too (the loop behind the peeled trial runs): some search of 2..19 evaluations
    assert any(v is not None and 1 < v < MAXFEV for s in seqs for v in s)
    return (x, f, g, p), seqs


def _same_bits(a, b, what):
    for name, u, v in zip(("x", "f", "g"), a[:3], b[:3]):
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64)), "%s: %s differs in rows %s" % (
            what, name, np.unique(np.nonzero(u.view(np.uint64) != v.view(np.uint64))[0])[:10])
    for k in FIELDS:
        u, v = a[3][k], b[3][k]
        same = u.view(np.uint64) == v.view(np.uint64) if u.dtype == np.float64 else u == v
        assert np.all(same), "%s: %s differs in rows %s" % (what, k, np.nonzero(~same)[0][:10])


def _run(solver, x0, force_general=False):
    import torch
    import cppnumericalsolvers_amd as amd
    n = x0.shape[1]
    dev = torch.from_numpy(np.ascontiguousarray(x0)).to("cuda:0")
    trace = amd.Trace([0], 4, n, dev.device, with_x=False) if force_general else None
    x, f, g, p = solver.minimize(amd.Rosenbrock(), dev, trace=trace)
    torch.cuda.synchronize()
    return (x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)), solver.last_launch()


@pytest.fixture
def capped(monkeypatch):
    """capped(cap): a fresh context whose resident grid is capped to `cap` workgroups (None: uncapped)."""
    import cppnumericalsolvers_amd as amd
    made = []

    def make(cap):
        if cap is None:
            monkeypatch.delenv(CAP_ENV, raising=False)
        else:
            monkeypatch.setenv(CAP_ENV, str(cap))
        ctx = amd.Context(0)
        monkeypatch.delenv(CAP_ENV, raising=False)
        made.append(ctx)
        return ctx

    yield make
    for ctx in made:
        ctx.close()


# configs[1]'s kernel (8 lanes x 4, six y columns) and configs[2]'s (16 lanes x 4, ten y columns)
@pytest.mark.parametrize("n,m,W", [(32, 6, 8), (64, 10, 16)])
def test_peeled_search_corners_equal_twin_and_general_kernel(capped, oracle, n, m, W):
    import cppnumericalsolvers_amd as amd
    x0, cls = corner_batch(oracle, n)
    twin, _ = prove_corners(oracle, x0, cls, m, 4)
    B, per_wave = len(x0), 64 // W
    assert B % per_wave != 0, B                              # a ragged last wavefront
    results = {}
    for cap in (1, 2, None):
        solver = amd.BatchedLbfgs(m=m, stopping_progress=amd.parity_stop(), context=capped(cap))
        lean, ll = _run(solver, x0)
        assert ll["kernel"] == "lean" and (ll["lanes_per_problem"], ll["elems_per_lane"], ll["y_columns_in_registers"]) == (W, 4, m), ll
        assert solver.last_arithmetic() == "fma"
        if cap is not None:
            assert ll["blocks"] == cap and B >= 4 * cap * per_wave * (ll["threads"] // 64), (ll, B)   # every segment re-fetches
        _same_bits(lean, twin, "lean kernel, cap %s, against the twin" % cap)
        results[cap] = lean
    general, ll = _run(amd.BatchedLbfgs(m=m, stopping_progress=amd.parity_stop(), context=capped(1)), x0, force_general=True)
    assert ll["kernel"] == "general" and ll["blocks"] == 1, ll
    _same_bits(results[1], general, "lean against the general kernel, cap 1")


def test_peeled_search_with_an_iteration_limit_and_variant_a(capped, oracle):
    """The thresholds stay kernel arguments: parity stopping with num_iterations = 3 (every solve is cut inside its
    first line searches, where the corner rows differ most) and variant A (x_delta = 1e-9), capped grid, n = 32."""
    import cppnumericalsolvers_amd as amd
    n, m = 32, 6
    x0, cls = corner_batch(oracle, n)
    for change in (dict(num_iterations=3), dict(x_delta=1e-9)):
        so, se = oracle.parity_stop(), amd.parity_stop()
        for k, v in change.items():
            setattr(so, k, v)
            setattr(se, k, v)
        twin = oracle.minimize_batch("rosenbrock", x0, m=m, stop=so, reduction="butterfly_fma", width=32, fma_group=4)
        solver = amd.BatchedLbfgs(m=m, stopping_progress=se, context=capped(1))
        lean, ll = _run(solver, x0)
        assert ll["kernel"] == "lean" and ll["blocks"] == 1, ll
        _same_bits(lean, twin, "lean kernel, %s" % change)
