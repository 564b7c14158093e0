"""Shapes, inputs and trajectories of the step audit (tests/step_lib.py): tests/test_step_lib.py runs every row on the CPU
twins, tests/test_gpu_steps_mpmath.py on the device.

Batches of 24 with 8 traced problems.  Stop record: an iteration limit of 3 m + 8, so that the ring wraps twice, and the
relative gradient test at 1e-6, so that a run ends before the rounding-level regime where every guard is undecidable; every
other test off.  Inputs: chained Rosenbrock from the `std` and `u2` starts, a convex diagonal quadratic with a spectrum
spread of 1e2, Rosenbrock in Second mode (diag H(x) of every iterate), the diagonal quadratic in Second mode with its constant
diagonal (device only: the oracle builds the constant diagonal for the ridge objective alone), the dense quartic example
functor (device only, direction and line search: the checks that need no definition of the objective).

A trajectory is x_0 .. x_T with the gradient and the value of every iterate.  Where the entry takes a trace it comes from
amd.Trace(with_x, with_g) in one launch; where it refuses one (the lean kernels, float32) and for every CPU twin it comes
from prefix-limited solves: iterate k is the result of the same solve limited to k - 1 iterations (the strict '>' of
progress.h:212), iterate 1 of a solve whose gradient test every point passes.
"""
import numpy as np

import hp_lib
import step_lib

B = 24
TRACED = (0, 3, 6, 9, 13, 16, 20, 23)
GRADIENT_NORM = 1e-6
SPREAD = 1e2


def limit(m):
    return 3 * m + 8


def stop_fields(num_iterations):
    return dict(num_iterations=num_iterations, x_delta=0.0, x_delta_violations=1, f_delta=0.0, f_delta_violations=1,
                f_delta_relative=0, gradient_norm=GRADIENT_NORM, gradient_norm_relative=1, past=0, past_delta=0.0)


def first_iteration_fields():
    """every point passes the gradient test: the solve ends after its first iteration"""
    return dict(stop_fields(1), gradient_norm=1e300)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def starts(kind, n, dtype="float64"):
    import cppnumericalsolvers_amd as amd
    x0 = amd.synthetic_x0_host(B, n, kind)
    return x0.astype(np.float32) if dtype == "float32" else x0


def diag_coefficients(n, dtype="float64"):
    """a_i from 1 to 1e2, geometric (n = 1: 1), and c = 0.25; exact in float32 where the kernel is the float one"""
    a = np.geomspace(1.0, SPREAD, n) if n > 1 else np.ones(1)
    if dtype == "float32":
        a = a.astype(np.float32).astype(np.float64)
    return a, 0.25


def objective(name, n, dtype="float64", sequential=False):
    """(params blob or None, evaluate(x) -> hp_lib.Eval, (k_f, k_g)): `sequential` counts the value's sum as a chain of n,
    the reference's order, where the kernels' k counts a tree"""
    if name in ("rosenbrock", "rosenbrock_second"):
        k_f, k_g, _ = hp_lib.rosenbrock_k(n)
        return None, hp_lib.rosenbrock, ((n + 5) if sequential else k_f, k_g)
    if name in ("diag_quadratic", "diag_quadratic_second"):
        a, c = diag_coefficients(n, dtype)
        k_f, k_g, _ = hp_lib.diag_quadratic_k(n)
        return np.concatenate([a, [c]]), (lambda x: hp_lib.diag_quadratic(x, a, c)), ((n + 3) if sequential else k_f, k_g)
    raise KeyError(name)


def hess_diag(name, n):
    """the 200-bit diagonal of the Hessian at x, for the Second-mode rows"""
    if name == "rosenbrock_second":     # H_jj = [j < n-1] (1200 x_j^2 - 400 x_{j+1} + 2) + [j > 0] 200 (tests/hp_lib.py)
        def diagonal(x):
            v = hp_lib.vec(x)
            return [(1200 * v[j] * v[j] - 400 * v[j + 1] + 2 if j + 1 < n else 0) + (200 if j > 0 else 0) for j in range(n)]
        return diagonal
    if name == "diag_quadratic_second":
        a, _ = diag_coefficients(n)
        return lambda x: [2 * hp_lib.mpf(float(v)) for v in a]
    return None


def dense_quartic(n):
    """parameters and 24 starts of the SPD family of tests/dense_cases.py"""
    import dense_cases
    ints = dense_cases.integers(31, n, rows=B)
    return dense_cases.params(ints), dense_cases.starts(ints)


def box(n, per_problem=False):
    """a box that cuts the Rosenbrock minimiser off; one per problem: the same box moved by up to 0.1"""
    lower, upper = np.full(n, -0.5), np.full(n, 0.8)
    if per_problem:
        shift = 0.1 * np.random.default_rng(n).uniform(0.0, 1.0, (B, 1))
        return lower - shift, upper + shift
    return lower, upper


def box_starts(kind, n, lower, upper):
    """the starts clipped into the box, the first two coordinates of every other problem ON a bound"""
    x0 = np.clip(starts(kind, n), lower, upper)
    lo, hi = np.broadcast_to(lower, x0.shape), np.broadcast_to(upper, x0.shape)
    x0[::2, 0] = lo[::2, 0]
    x0[::2, 1 % n] = hi[::2, 1 % n]
    return x0


# ---- rows ----------------------------------------------------------------------------------------------------------------------
# (objective, start, n, m)
# (n = 2 keeps to m <= 3: six pairs in a plane cancel so far that the slack of g^T d passes g^T d itself before the
# gradient test ends the run)
LBFGS_SHAPES = (("rosenbrock", "std", 2, 1), ("rosenbrock", "u2", 2, 3), ("rosenbrock", "std", 7, 3),
                ("rosenbrock", "u2", 8, 6), ("rosenbrock", "std", 9, 1), ("rosenbrock", "std", 17, 6),
                ("rosenbrock", "u2", 33, 3), ("rosenbrock", "std", 64, 3), ("rosenbrock", "std", 100, 3),
                ("rosenbrock", "std", 256, 1), ("diag_quadratic", "std", 7, 3), ("diag_quadratic", "u2", 17, 1),
                ("diag_quadratic", "std", 64, 6), ("rosenbrock_second", "std", 8, 3), ("rosenbrock_second", "u2", 33, 6))
WIDE_SHAPE = ("rosenbrock", "std", 300, 1)
# every built (lanes per problem, coordinates per lane) that covers the n of a mapping row
MAPPINGS = ((8, 1), (8, 2), (8, 4), (16, 1), (16, 2), (16, 4), (32, 2), (32, 4), (64, 1), (64, 2), (64, 4))
MAPPING_SHAPES = (("rosenbrock", "std", 8, 6), ("rosenbrock", "u2", 33, 3), ("rosenbrock", "std", 64, 3),
                  ("rosenbrock", "std", 256, 1))
PLACEMENTS = (1, 2)                      # MI355_HISTORY_LDS, MI355_HISTORY_Y_IN_REGISTERS
HZ_SHAPES = (("rosenbrock", "std", 7, 3), ("rosenbrock", "u2", 33, 6), ("diag_quadratic", "std", 17, 1))
LEAN_SHAPE = ("rosenbrock", "std", 32, 6)
# float32: u = 2^-24 leaves the reset decision (the counted slack of g^T d against g^T d itself) undecidable with six pairs on
# Rosenbrock, and with three from the `std` starts; these rows stay decidable (tests/test_step_lib.py)
F32_SHAPES = (("rosenbrock", "std", 9, 1), ("rosenbrock", "u2", 17, 3), ("rosenbrock", "u2", 33, 3),
              ("diag_quadratic", "std", 17, 6), ("rosenbrock", "u2", 100, 3))
BFGS_SHAPES = (("rosenbrock", "std", 7), ("rosenbrock", "u2", 32))
# Dense Bfgs has no ring and never drops a pair: the counted chain behind H grows with every update, and from about the
# 18th on the slack of g^T H g passes g^T H g itself.  Its rows run under the limit and the caps of m = 2 (15 iterations).
BFGS_M = 2
LBFGSB_SHAPES = (("rosenbrock", "std", 7, 3), ("rosenbrock", "u2", 33, 5))
DENSE_QUARTIC_SHAPES = ((7, 3), (16, 6))


def lbfgs_rows(families, extra=()):
    """(family, objective, start, n, m) of the Lbfgs rows; the fused kernels are built for First mode up to n = 256"""
    return [(f,) + r for r in LBFGS_SHAPES + tuple(extra) + (WIDE_SHAPE,) for f in families
            if not (f == "fma" and (r[2] > 256 or r[0].endswith("_second")))]


def width(n):
    return 1 << max(3, int(np.ceil(np.log2(n))))


def mappings_of(n):
    """the built mappings from the padded width of n to four times it"""
    return [(W, E) for W, E in MAPPINGS if width(n) <= W * E <= 4 * width(n)]


# ---- trajectories ------------------------------------------------------------------------------------------------------------
def prefix_trajectories(solve, x0, f0, g0, m, fields=None, first_fields=None):
    """solve(x0 rows, stop fields) -> (x, f, g, progress) -> [(xs, gs, fs)] per row of x0; `fields`, `first_fields`: another
    stop record than this module's"""
    fields, first_fields = fields or stop_fields, first_fields or first_iteration_fields
    rows = x0.shape[0]
    out = [([x0[b]], [g0[b]], [f0[b]]) for b in range(rows)]
    running = list(range(rows))
    for k in range(1, limit(m) + 2):
        if not running:
            break
        x, f, g, p = solve(x0[running], first_fields() if k == 1 else fields(k - 1))
        still = []
        for i, b in enumerate(running):
            done = int(p["num_iterations"][i])
            assert done <= k, "a solve limited to %d iterations took %d" % (k - 1, done)
            if done == k:
                out[b][0].append(x[i])
                out[b][1].append(g[i])
                out[b][2].append(f[i])
                still.append(b)
            else:             # it ended sooner, on the gradient test: the iterate it ended on is the one recorded last
                assert done == k - 1 and np.array_equal(x[i], out[b][0][-1]), "a prefix-limited solve took another path"
        running = still
    return [(np.array(xs), np.array(gs), np.array(fs)) for xs, gs, fs in out]


def trace_trajectories(trace, x0, f0, g0, dtype=np.float64):
    """the records of an amd.Trace of the rows TRACED -> [(xs, gs, fs)]"""
    out = []
    for i in range(len(trace.problems)):
        rec, tx, tg = trace.history(i)
        assert np.array_equal(rec["num_iterations"], np.arange(1, len(rec) + 1)), "the trace kept every iteration"
        out.append((np.concatenate([x0[i:i + 1], tx]).astype(dtype), np.concatenate([g0[i:i + 1], tg]).astype(dtype),
                    np.concatenate([f0[i:i + 1], rec["value"]]).astype(dtype)))
    return out


def rules_of(family, m, **kw):
    """step_lib.Rules of a kernel family: how deep its inner products are.  "fused": a lane's four coordinates are a chain
    of four fused links where the tree has a product and two levels — one deeper (tests/hp_lib.py, diag_quadratic_k)."""
    return step_lib.Rules(m, dot={"reference": "sequential", "fma": "fused"}.get(family, "tree"), **kw)


_AUDITED = {}


def audit_once(trajectories, rules, *args, **kw):
    """step_lib.audit_case, kept per trajectory: the kernels promise the same bits on every mapping and history placement,
    and the audit is a function of the trajectory alone.  (A mapping whose bits differ is audited on its own.)"""
    import hashlib
    h = hashlib.sha256(repr((rules.m, rules.dtype, rules.linesearch, rules.solver, rules.second, rules.dot)).encode())
    for xs, gs, fs in trajectories:
        for a in (xs, gs, fs):
            h.update(np.ascontiguousarray(a).tobytes())
    key = h.hexdigest()
    if key not in _AUDITED:
        _AUDITED[key] = step_lib.audit_case(trajectories, rules, *args, **kw)
    return _AUDITED[key]


def assert_case(report, m, what):
    """the bounds and the two caps; returns the report's line for the summary"""
    line = "%s: %s" % (what, report.line())
    assert not report.bad, "%s\n%d outside their bound, first: %s" % (line, len(report.bad), report.bad[:3])
    broken = step_lib.caps(report, m)
    assert not broken, "%s\n%s\nundecidable: %s\nexceptions: %s" % (line, broken, report.undecidable[:4],
                                                                       report.exception_notes[:4])
    return line
