"""What the float ask/tell tests share (tests/test_ask_tell_f32_cpu.py, tests/test_gpu_ask_tell_f32.py): float32 starts,
the stop records as the engine's capi.Stop, the bitwise comparison, and the inputs of the torch-objective test with the
seed they are committed under.  TEST INFRASTRUCTURE: only tests/ imports this module."""
import os

import numpy as np

import at_lib
import l32_lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(HERE, "ask_tell_f32")
B = 131   # not a multiple of the segments per wavefront (8, 4, 2) and more than one wavefront at every mapping
MAPPINGS = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))
GRADIENT_STATUS = 4
SYMBOLS = tuple("mi355_lbfgs_ask_tell_f32_" + s for s in ("create", "x", "step", "active", "results", "destroy"))


def starts(objective, count, n, seed):
    """the starts of the fp64 ask/tell tests, rounded to float32"""
    return np.ascontiguousarray(at_lib.starts(objective, count, n, seed), dtype=np.float32)


def hostile_starts(n):
    """NaN, +inf, -inf and 1e30 coordinates, whole rows of them, and rows already at Rosenbrock's minimiser (the search is
    refused at once there: g = 0)"""
    base = starts("rosenbrock", 4, n, seed=5)
    rows = [np.full(n, np.nan), np.full(n, np.inf), np.full(n, -np.inf), np.full(n, 1e30), np.full(n, -1e30)]
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30)):
        r = base[k].copy()
        r[k % n] = v
        rows.append(r)
    rows += [np.ones(n), np.ones(n), np.ones(n)]
    return np.ascontiguousarray(np.stack(rows), dtype=np.float32)


def capi_stop(record):
    """an l32_lib stop record (STOP_DTYPE) as the engine's capi.Stop"""
    from cppnumericalsolvers_amd import capi
    s = capi.Stop()
    for name in L.STOP_DTYPE.names:
        setattr(s, name, record[name][0].item())
    return s


def assert_same(got, want, what):
    """x, f, g (float32) and every progress field, byte for byte"""
    for name, a, b in zip(("x", "f", "g"), got[:3], want[:3]):
        assert a.dtype == np.float32 and b.dtype == np.float32, "%s: %s is not float32" % (what, name)
        if a.tobytes() != b.tobytes():
            rows = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(want[1]), -1).any(axis=1))[0]
            raise AssertionError("%s: %s differs on %d problems, first %s" % (what, name, len(rows), rows[:8].tolist()))
    for fld in L.PROGRESS_FIELDS:
        a, b = np.ascontiguousarray(got[3][fld]), np.ascontiguousarray(want[3][fld])
        if a.tobytes() != b.tobytes():
            rows = np.nonzero((a.view(np.uint8) != b.view(np.uint8)).reshape(len(a), -1).any(axis=1))[0]
            raise AssertionError("%s: progress.%s differs on %d problems, first %s: %s vs %s"
                                 % (what, fld, len(rows), rows[:8].tolist(), a[rows[:4]], b[rows[:4]]))


# ---- the torch-objective test: f_b(x) = 1/2 sum_i a_i (x_i - c_{b,i})^2 in float32 -------------------------------------
QUAD_SEED = 20261020
QUAD_N, QUAD_M = 13, 6
QUAD_TAU = 1e-4


def quadratic_inputs():
    """(a [n] in [0.5, 2], c [B, n] in [-2, 2], x0 [B, n] in [-3, 3]), float32, from the committed seed"""
    rng = np.random.default_rng(QUAD_SEED)
    a = rng.uniform(0.5, 2.0, QUAD_N).astype(np.float32)
    c = rng.uniform(-2.0, 2.0, (B, QUAD_N)).astype(np.float32)
    x0 = rng.uniform(-3.0, 3.0, (B, QUAD_N)).astype(np.float32)
    return a, c, x0


def quadratic_stop_fields():
    """only the absolute gradient test at tau and the iteration limit"""
    return dict(num_iterations=200, x_delta=0.0, x_delta_violations=1, f_delta=0.0, f_delta_violations=1,
                f_delta_relative=0, gradient_norm=QUAD_TAU, gradient_norm_relative=0, past=0, past_delta=0.0)
