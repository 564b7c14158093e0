"""ctypes helpers of the trust-region tests: the CPU twin (tests/trust_region/tr_twin.hpp, built by build() into
tests/trust_region/_build/) and, where the reference tree exists, the reference harness compiled into a directory the
caller names (tests/trust_region/ref_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TR_DIR = os.path.join(HERE, "trust_region")
REPO = os.path.dirname(HERE)
REFERENCE = "/root/reference"
TWIN_LIB = os.path.join(TR_DIR, "_build", "libtr_twin.so")

ROSENBROCK, DIAG_QUADRATIC, QUARTIC, DENSE = 0, 1, 100, 101
REF_ORDER, DEVICE_ORDER = 0, 1

STOP_DTYPE = np.dtype([("num_iterations", "<u8"), ("x_delta", "<f8"), ("x_delta_violations", "<i4"), ("f_delta", "<f8"),
                       ("f_delta_violations", "<i4"), ("f_delta_relative", "<i4"), ("gradient_norm", "<f8"),
                       ("gradient_norm_relative", "<i4"), ("past", "<i4"), ("past_delta", "<f8")], align=True)
CONFIG_FIELDS = ("initial_radius", "max_radius", "acceptance_threshold", "shrink_factor", "expand_factor", "rho_low",
                 "rho_high", "cg_forcing_coefficient", "cg_max_iterations_floor", "min_radius", "rejection_retry_limit")
CONFIG_DTYPE = np.dtype([(f, "<i4" if f in ("cg_max_iterations_floor", "rejection_retry_limit") else "<f8")
                         for f in CONFIG_FIELDS], align=True)
PROGRESS_DTYPE = np.dtype([("status", "<i4"), ("num_iterations", "<u4"), ("nfev", "<u4"), ("sum_k", "<u4"),
                           ("x_delta", "<f8"), ("f_delta", "<f8"), ("gradient_norm", "<f8")], align=True)
COUNTERS_DTYPE = np.dtype([("max_cg_iterations", "<u4"), ("subproblems_of_3_cg_iterations", "<u4"),
                           ("negative_curvature_exits", "<u4"), ("boundary_hits", "<u4"), ("conditions", "<u4"),
                           ("min_condition_margin", "<f8")], align=True)
NO_MUTATION, PRODUCT_WALKS_COLUMN = 0, 1    # tr_twin::Mutation
DEFAULT_CONFIG = dict(initial_radius=1.0, max_radius=1e10, acceptance_threshold=0.15, shrink_factor=0.25,
                      expand_factor=2.0, rho_low=0.25, rho_high=0.75, cg_forcing_coefficient=0.5,
                      cg_max_iterations_floor=10, min_radius=1e-12, rejection_retry_limit=50)
# the stopping presets: DefaultStoppingSolverProgress, ConservativeStoppingSolverProgress (progress.h; as
# mi355_lbfgs_default_stop fills them) and the package's parity preset (cppnumericalsolvers_amd.parity_stop)
_DEFAULT = dict(num_iterations=10000, x_delta=1e-9, x_delta_violations=1, f_delta=0.0, f_delta_violations=1,
                f_delta_relative=0, gradient_norm=1e-5, gradient_norm_relative=1, past=3, past_delta=1e-6)
STOP_PRESETS = {
    "default": _DEFAULT,
    "conservative": {**_DEFAULT, "gradient_norm": 5e-6, "past": 5, "past_delta": 1e-10},
    "parity": {**_DEFAULT, "x_delta": 1e-11, "gradient_norm": 1e-8, "past": 0},
}


def make_stop(**kw):
    s = np.zeros(1, dtype=STOP_DTYPE)
    for k, v in kw.items():
        s[k] = v
    return s


def make_config(**kw):
    c = np.zeros(1, dtype=CONFIG_DTYPE)
    for k, v in {**DEFAULT_CONFIG, **kw}.items():
        c[k] = v
    return c


def _solve(fn, objective, x0, params, stop, config, condition_stop, extra):
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B, n = x0.shape
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B)
    prog = np.zeros(B, dtype=PROGRESS_DTYPE)
    rc = fn(objective, n, B, params.ctypes.data, stop.ctypes.data, C.c_double(condition_stop), config.ctypes.data,
            *extra, x0.ctypes.data, x.ctypes.data, f.ctypes.data, g.ctypes.data, prog.ctypes.data)
    assert rc == 0, "unsupported solve"
    return x, f, g, prog


def _declare(fn, n_extra):
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p] + [C.c_int] * n_extra + \
                  [C.c_void_p] * 5
    return fn


_twin = None


def twin_solve(objective, x0, params=None, stop=None, config=None, condition_stop=0.0, order=REF_ORDER, W=None):
    """The CPU twin: (x, f, g, progress) of every row of x0.  W: the padded width of the device order (default: the
    library's mapping, the next power of two >= max(n, 8))."""
    global _twin
    if _twin is None:
        _twin = _declare(C.CDLL(TWIN_LIB).tr_twin_solve, 2)
    n = np.asarray(x0).shape[1]
    if W is None:
        W = 8
        while W < n:
            W *= 2
    return _solve(_twin, objective, x0, params, stop if stop is not None else make_stop(**STOP_PRESETS["default"]),
                  config if config is not None else make_config(), condition_stop, (order, W))


_twin_ex = None


def twin_solve_ex(objective, x0, params=None, stop=None, config=None, condition_stop=0.0, order=REF_ORDER, W=None,
                  mutation=NO_MUTATION):
    """twin_solve with the twin's counters as a fifth result and, mutation = PRODUCT_WALKS_COLUMN, its deliberate bug
    planted (H d walking a column of H for a row)."""
    global _twin_ex
    if _twin_ex is None:
        _twin_ex = C.CDLL(TWIN_LIB).tr_twin_solve_ex
        _twin_ex.restype = C.c_int
        _twin_ex.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p] + \
                            [C.c_int] * 3 + [C.c_void_p] * 6
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B, n = x0.shape
    if W is None:
        W = 8
        while W < n:
            W *= 2
    stop = stop if stop is not None else make_stop(**STOP_PRESETS["default"])
    config = config if config is not None else make_config()
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B)
    prog, cnt = np.zeros(B, dtype=PROGRESS_DTYPE), np.zeros(B, dtype=COUNTERS_DTYPE)
    rc = _twin_ex(objective, n, B, params.ctypes.data, stop.ctypes.data, C.c_double(condition_stop), config.ctypes.data,
                  order, W, mutation, x0.ctypes.data, x.ctypes.data, f.ctypes.data, g.ctypes.data, prog.ctypes.data,
                  cnt.ctypes.data)
    assert rc == 0, "unsupported solve"
    return x, f, g, prog, cnt


def build_reference(out_dir):
    """Compile the reference harness over the reference tree into out_dir; returns the library path."""
    lib = os.path.join(out_dir, "libtr_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                           "-I" + os.path.join(TR_DIR, "overlay"), "-I" + os.path.join(REPO, "oracle", "eigen_shim"),
                           "-I" + os.path.join(REFERENCE, "include"), "-I" + TR_DIR,
                           os.path.join(TR_DIR, "ref_harness.cpp"), "-o", lib])
    return lib


def reference_trajectory(lib_path, objective, x0, params=None, stop=None, config=None, condition_stop=0.0,
                         capacity=1000):
    """One reference solve from x0 (a single start) with its per-iteration states from the reference's step callback:
    (x, f, g, progress, rows [K, 6] = num_iterations, status, value, x_delta, f_delta, gradient_norm, xs [K, n])."""
    fn = C.CDLL(lib_path).tr_ref_trajectory
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p] + [C.c_void_p] * 5 + \
                  [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(1, -1))
    n = x0.shape[1]
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    stop = stop if stop is not None else make_stop(**STOP_PRESETS["default"])
    config = config if config is not None else make_config()
    x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(1)
    prog = np.zeros(1, dtype=PROGRESS_DTYPE)
    rows, xs, count = np.zeros((capacity, 6)), np.zeros((capacity, n)), C.c_int(0)
    rc = fn(objective, n, params.ctypes.data, stop.ctypes.data, C.c_double(condition_stop), config.ctypes.data,
            x0.ctypes.data, x.ctypes.data, f.ctypes.data, g.ctypes.data, prog.ctypes.data, capacity, rows.ctypes.data,
            xs.ctypes.data, C.byref(count))
    assert rc == 0, "unsupported solve"
    k = count.value
    return x, f, g, prog, rows[:k].copy(), xs[:k].copy()


def reference_solver(lib_path):
    fn = _declare(C.CDLL(lib_path).tr_ref_solve, 0)

    def solve(objective, x0, params=None, stop=None, config=None, condition_stop=0.0):
        return _solve(fn, objective, x0, params, stop if stop is not None else make_stop(**STOP_PRESETS["default"]),
                      config if config is not None else make_config(), condition_stop, ())
    return solve
