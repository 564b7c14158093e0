"""ctypes helpers of the first-order tests (GradientDescent, ConjugatedGradientDescent): the CPU twin
(tests/first_order/fo_twin.hpp, built by build() into tests/first_order/_build/) and, where the reference tree exists,
the reference harness compiled into a directory the caller names (tests/first_order/ref_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FO_DIR = os.path.join(HERE, "first_order")
REPO = os.path.dirname(HERE)
REFERENCE = "/root/reference"
TWIN_LIB = os.path.join(FO_DIR, "_build", "libfo_twin.so")

GRADIENT_DESCENT, CONJUGATED_GRADIENT_DESCENT = 0, 1
METHOD_NAMES = {GRADIENT_DESCENT: "gd", CONJUGATED_GRADIENT_DESCENT: "cg"}
ROSENBROCK, DIAG_QUADRATIC, QUARTIC = 0, 1, 100
REF_ORDER, DEVICE_ORDER = 0, 1

STOP_DTYPE = np.dtype([("num_iterations", "<u8"), ("x_delta", "<f8"), ("x_delta_violations", "<i4"), ("f_delta", "<f8"),
                       ("f_delta_violations", "<i4"), ("f_delta_relative", "<i4"), ("gradient_norm", "<f8"),
                       ("gradient_norm_relative", "<i4"), ("past", "<i4"), ("past_delta", "<f8")], align=True)
CONFIG_FIELDS = ("c", "rho", "alpha_min")
CONFIG_DTYPE = np.dtype([(f, "<f8") for f in CONFIG_FIELDS], align=True)
PROGRESS_DTYPE = np.dtype([("status", "<i4"), ("num_iterations", "<u4"), ("nfev", "<u4"), ("sum_k", "<u4"),
                           ("x_delta", "<f8"), ("f_delta", "<f8"), ("gradient_norm", "<f8")], align=True)
COUNTERS_DTYPE = np.dtype([("max_trials", "<u4"), ("alpha_one_steps", "<u4"), ("alpha_less_steps", "<u4"),
                           ("alpha_min_exits", "<u4"), ("refused_searches", "<u4")], align=True)
DEFAULT_CONFIG = dict(c=0.2, rho=0.9, alpha_min=1e-8)   # linesearch/armijo.h:49-50, :56
# the stopping presets: DefaultStoppingSolverProgress (progress.h; as mi355_lbfgs_default_stop fills it) and the
# package's parity preset (cppnumericalsolvers_amd.parity_stop)
_DEFAULT = dict(num_iterations=10000, x_delta=1e-9, x_delta_violations=1, f_delta=0.0, f_delta_violations=1,
                f_delta_relative=0, gradient_norm=1e-5, gradient_norm_relative=1, past=3, past_delta=1e-6)
STOP_PRESETS = {
    "default": _DEFAULT,
    "parity": {**_DEFAULT, "x_delta": 1e-11, "gradient_norm": 1e-8, "past": 0},
}
# alpha *= 0.9 from 1 first reaches alpha <= 1e-8 after 175 multiplications: the longest Armijo search has 176 trials
MAX_ARMIJO_TRIALS = 176


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


def library_mapping(n):
    """(W, E) the library picks for lanes_per_problem = 0."""
    W = 8
    while W < n and W < 64:
        W *= 2
    return W, (1 if n <= W else (2 if n <= 2 * W else 4))


def padded_width(n):
    W, E = library_mapping(n)
    return W * E


def _solve(fn, method, objective, x0, params, stop, config, extra, counters=False):
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B, n = x0.shape
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B)
    prog = np.zeros(B, dtype=PROGRESS_DTYPE)
    tail = []
    if counters:
        cnt = np.zeros(B, dtype=COUNTERS_DTYPE)
        tail = [cnt.ctypes.data]
    rc = fn(method, objective, n, B, params.ctypes.data, stop.ctypes.data, config.ctypes.data, *extra, x0.ctypes.data,
            x.ctypes.data, f.ctypes.data, g.ctypes.data, prog.ctypes.data, *tail)
    assert rc == 0, "unsupported solve"
    return (x, f, g, prog, cnt) if counters else (x, f, g, prog)


def _declare(fn, n_extra, n_tail):
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * n_extra + \
                  [C.c_void_p] * (5 + n_tail)
    return fn


def _declare_trajectory(fn, n_extra):
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * n_extra + \
                  [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


_twin = None


def _twin_lib():
    global _twin
    if _twin is None:
        _twin = C.CDLL(TWIN_LIB)
        _declare(_twin.fo_twin_solve, 2, 1)
        _declare_trajectory(_twin.fo_twin_trajectory, 2)
    return _twin


def twin_solve(method, objective, x0, params=None, stop=None, config=None, order=REF_ORDER, width=None, counters=False):
    """The CPU twin: (x, f, g, progress[, counters]) of every row of x0.  width: W x E of the device order (default: the
    library's mapping)."""
    n = np.asarray(x0).shape[1]
    out = _solve(_twin_lib().fo_twin_solve, method, objective, x0, params,
                 stop if stop is not None else make_stop(**STOP_PRESETS["default"]),
                 config if config is not None else make_config(),
                 (order, width if width is not None else padded_width(n)), counters=True)
    return out if counters else out[:4]


def _trajectory(fn, extra, method, objective, x0, params, stop, config, capacity):
    x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(1, -1))
    n = x0.shape[1]
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    stop = stop if stop is not None else make_stop(**STOP_PRESETS["default"])
    config = config if config is not None else make_config()
    x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(1)
    prog = np.zeros(1, dtype=PROGRESS_DTYPE)
    rows, xs, count = np.zeros((capacity, 6)), np.zeros((capacity, n)), C.c_int(0)
    rc = fn(method, objective, n, params.ctypes.data, stop.ctypes.data, config.ctypes.data, *extra, x0.ctypes.data,
            x.ctypes.data, f.ctypes.data, g.ctypes.data, prog.ctypes.data, capacity, rows.ctypes.data, xs.ctypes.data,
            C.byref(count))
    assert rc == 0, "unsupported solve"
    k = count.value
    return x, f, g, prog, rows[:k].copy(), xs[:k].copy()


def twin_trajectory(method, objective, x0, params=None, stop=None, config=None, order=REF_ORDER, width=None,
                    capacity=1000):
    """One twin solve from x0 (a single start) with its per-iteration states: (x, f, g, progress, rows [K, 6] =
    num_iterations, status, value, x_delta, f_delta, gradient_norm, xs [K, n])."""
    n = np.asarray(x0).reshape(1, -1).shape[1]
    return _trajectory(_twin_lib().fo_twin_trajectory, (order, width if width is not None else padded_width(n)), method,
                       objective, x0, params, stop, config, capacity)


def build_reference(out_dir):
    """Compile the reference harness over the reference tree into out_dir; returns the library path.  (The Eigen
    stand-in covers everything the two solver headers and their searches use: no overlay is needed.)"""
    lib = os.path.join(out_dir, "libfo_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                           "-I" + os.path.join(REPO, "oracle", "eigen_shim"),
                           "-I" + os.path.join(REFERENCE, "include"), "-I" + FO_DIR,
                           os.path.join(FO_DIR, "ref_harness.cpp"), "-o", lib])
    return lib


def reference_trajectory(lib_path, method, objective, x0, params=None, stop=None, config=None, capacity=1000):
    """One reference solve from x0 with the states its step callback sees (as twin_trajectory)."""
    return _trajectory(_declare_trajectory(C.CDLL(lib_path).fo_ref_trajectory, 0), (), method, objective, x0, params,
                       stop, config, capacity)


def reference_solver(lib_path):
    fn = _declare(C.CDLL(lib_path).fo_ref_solve, 0, 0)

    def solve(method, objective, x0, params=None, stop=None, config=None):
        return _solve(fn, method, objective, x0, params,
                      stop if stop is not None else make_stop(**STOP_PRESETS["default"]),
                      config if config is not None else make_config(), ())
    return solve


def twin_solve_threaded(method, objective, x0, params=None, stop=None, config=None, order=REF_ORDER, width=None,
                        threads=8):
    """twin_solve over chunks of rows on `threads` host threads (the C call releases the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B = x0.shape[0]
    _twin_lib()
    bounds = np.linspace(0, B, 4 * threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda i: twin_solve(method, objective, x0[bounds[i]:bounds[i + 1]], params, stop, config,
                                                   order=order, width=width), range(4 * threads)))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
