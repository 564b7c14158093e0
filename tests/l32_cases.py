"""The cases of the float L-BFGS tests and their recorded reference results (tests/golden/lbfgs_f32_reference.npz,
written by tests/golden/make_golden_f32.py).

A case is built from its name and a seed alone: Rosenbrock / DiagQuadratic, n, m, a stopping record and two starts from
the synthetic_x0_host kinds ("std" and the wide kind), cast to float32; DiagQuadratic's a in [0.5, 50] from the same
generator.  The file therefore holds only outputs: per case f and the progress records in full, the SHA-256 digests of
x, g and of the per-iteration rows and iterates of start 0, and — for the cases GPU test 5 compares as numbers (every
DiagQuadratic case and the two 2-D Rosenbrock starts of the reference's verify.cc) — x in full."""
import hashlib
import os

import numpy as np

import l32_lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbfgs_f32_reference.npz")
RECORDED_SEED = 20261019
DIMS = (2, 5, 8, 13, 33, 64, 65, 130)
HISTORIES = (1, 3, 6, 10)
_ZERO = dict(num_iterations=40, x_delta=0.0, x_delta_violations=1, f_delta=0.0, f_delta_violations=1, f_delta_relative=0,
             gradient_norm=0.0, gradient_norm_relative=1, past=0, past_delta=0.0)
STOPS = {
    "default": L.STOP_PRESETS["default"],
    "conservative": L.STOP_PRESETS["conservative"],
    "past0": {**L.STOP_PRESETS["default"], "past": 0},
    "iters1": {**L.STOP_PRESETS["default"], "num_iterations": 1},
    "iters2": {**L.STOP_PRESETS["default"], "num_iterations": 2},
    "iters3": {**L.STOP_PRESETS["default"], "num_iterations": 3},
    "iters7": {**L.STOP_PRESETS["default"], "num_iterations": 7},
    "zero40": _ZERO,
}
VERIFY_STARTS = np.array([[15.0, 8.0], [-1.0, 2.0]], dtype=np.float32)   # src/test/verify.cc:23,129
VERIFY_BOUND = 1e-4
# The gap between the twin's two summation orders (reference order against the device's pairwise tree) over the cases
# compared as numbers, measured on the recorded draw by tests/test_lbfgs_f32_twin.py::test_gap_between_the_two_orders:
# max |dx|_inf = 3.3945e-4 (diag_quadratic_n130_m1_default), max |df| = 1.0681e-4.  Float solves stop on the plateau test
# at different iterates in the two orders; a = 50 at |x| ~ 1e-3 accounts for the size.
ORDER_GAP_X = 3.3945240e-4
ORDER_GAP_F = 1.0681153e-4


def _x0_host(B, n, kind, seed):
    from cppnumericalsolvers_amd.engine import synthetic_x0_host
    return synthetic_x0_host(B, n, kind, seed)


def _starts(n, seed):
    return np.concatenate([_x0_host(1, n, "std", seed), _x0_host(1, n, "wide", seed + 1)]).astype(np.float32)


def _coefficients(n, seed):
    u = (_x0_host(1, n, "wide", seed + 2)[0] + 2.0) / 4.0
    return np.concatenate([0.5 + 49.5 * u, [0.25]])


def grid_cases(seed=RECORDED_SEED):
    out = []
    for objective, tag in ((L.ROSENBROCK, "rosenbrock"), (L.DIAG_QUADRATIC, "diag_quadratic")):
        for n in DIMS:
            for m in HISTORIES:
                for stop_name, stop in STOPS.items():
                    s = seed + 1000 * n + 10 * m
                    out.append(dict(name="%s_n%d_m%d_%s" % (tag, n, m, stop_name), objective=objective, n=n, m=m,
                                    stop=L.make_stop(**stop), x0=_starts(n, s),
                                    params=_coefficients(n, s) if objective == L.DIAG_QUADRATIC else None))
    return out


def special_cases():
    d = L.default_stop()
    return [dict(name="verify_2d", objective=L.ROSENBROCK, n=2, m=10, stop=d, x0=VERIFY_STARTS.copy(), params=None),
            dict(name="overflow_n8", objective=L.ROSENBROCK, n=8, m=6, stop=d, x0=np.full((1, 8), 1e20, dtype=np.float32),
                 params=None)]


def all_cases(seed=RECORDED_SEED):
    return grid_cases(seed) + special_cases()


def compared_as_numbers(case):
    """the cases GPU test 5 and CPU test 3 compare on |x - x_ref| and |f - f_ref|"""
    return case["objective"] == L.DIAG_QUADRATIC or case["name"] == "verify_2d"


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def record_of(case, x, f, g, prog, rows, xs):
    """what the file keeps of one case's reference results"""
    r = {"f": f, "progress": prog, "x_sha256": digest(x), "g_sha256": digest(g), "rows_sha256": digest(rows),
         "xs_sha256": digest(xs), "iterations0": np.array([len(rows)], dtype=np.int32)}
    if compared_as_numbers(case):
        r["x"] = x
    return r


def same_record(case, got, want):
    """names of the fields of two records that differ (bytes; progress field by field, NaN equal to NaN)"""
    bad = []
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if k == "progress":
            for fld in L.PROGRESS_FIELDS:
                if not np.array_equal(a[fld], b[fld], equal_nan=a[fld].dtype.kind == "f"):
                    bad.append("progress." + fld)
        elif a.tobytes() != b.tobytes():
            bad.append(k)
    return bad


FIELDS = ("f", "progress", "x_sha256", "g_sha256", "rows_sha256", "xs_sha256", "iterations0", "x")


def pack(cases, records):
    """{case name: record} -> one array per field, the cases' arrays end to end in the order of `cases` (a zip member per
    array would cost more bytes than most of these arrays hold)"""
    out = {}
    for k in FIELDS:
        parts = [np.asarray(records[c["name"]][k]).reshape(-1) for c in cases if k in records[c["name"]]]
        a = np.concatenate(parts)
        out[k] = a.view(np.uint8) if k == "progress" else a
    return out


def load_recorded(cases=None):
    """{case name: record} of the recorded file, split by the shapes the case list gives"""
    cases = cases if cases is not None else all_cases()
    z = np.load(GOLDEN)
    blobs = {k: (z[k].view(L.PROGRESS_DTYPE) if k == "progress" else z[k]) for k in FIELDS}
    at = dict.fromkeys(FIELDS, 0)
    out = {}

    def take(k, count, shape):
        a = blobs[k][at[k]:at[k] + count].reshape(shape)
        at[k] += count
        return a
    for c in cases:
        R, n = c["x0"].shape
        r = {"f": take("f", R, (R,)), "progress": take("progress", R, (R,)), "iterations0": take("iterations0", 1, (1,))}
        for k in ("x_sha256", "g_sha256", "rows_sha256", "xs_sha256"):
            r[k] = take(k, 32, (32,))
        if compared_as_numbers(c):
            r["x"] = take("x", R * n, (R, n))
        out[c["name"]] = r
    assert all(at[k] == len(blobs[k]) for k in FIELDS), "the recorded file does not match the case list"
    return out
