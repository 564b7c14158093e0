"""ctypes helpers of the float L-BFGS tests: the CPU twin (tests/lbfgs_f32/f32_twin.hpp, built by build() into
tests/lbfgs_f32/_build/) and, where the reference tree exists, the reference harness compiled into a directory the
caller names (tests/lbfgs_f32/ref_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L32_DIR = os.path.join(HERE, "lbfgs_f32")
REPO = os.path.dirname(HERE)
REFERENCE = "/root/reference"
TWIN_LIB = os.path.join(L32_DIR, "_build", "libf32_twin.so")

ROSENBROCK, DIAG_QUADRATIC = 0, 1
REF_ORDER, DEVICE_ORDER = 0, 1

STOP_DTYPE = np.dtype([("num_iterations", "<u8"), ("x_delta", "<f8"), ("x_delta_violations", "<i4"), ("f_delta", "<f8"),
                       ("f_delta_violations", "<i4"), ("f_delta_relative", "<i4"), ("gradient_norm", "<f8"),
                       ("gradient_norm_relative", "<i4"), ("past", "<i4"), ("past_delta", "<f8")], align=True)
PROGRESS_DTYPE = np.dtype([("status", "<i4"), ("num_iterations", "<u4"), ("nfev", "<u4"), ("sum_k", "<u4"),
                           ("x_delta", "<f8"), ("f_delta", "<f8"), ("gradient_norm", "<f8")], align=True)
PROGRESS_FIELDS = ("status", "num_iterations", "nfev", "sum_k", "x_delta", "f_delta", "gradient_norm")
# the reference's presets (solver/progress.h: DefaultStoppingSolverProgress, ConservativeStoppingSolverProgress)
_DEFAULT = dict(num_iterations=10000, x_delta=1e-9, x_delta_violations=1, f_delta=0.0, f_delta_violations=1,
                f_delta_relative=0, gradient_norm=1e-5, gradient_norm_relative=1, past=3, past_delta=1e-6)
STOP_PRESETS = {
    "default": _DEFAULT,
    "conservative": {**_DEFAULT, "gradient_norm": 5e-6, "past": 5, "past_delta": 1e-10},
}


def make_stop(**kw):
    s = np.zeros(1, dtype=STOP_DTYPE)
    for k, v in kw.items():
        s[k] = v
    return s


def library_mapping(n):
    """(W, E) the library picks for lanes_per_problem = 0."""
    W = 8
    while W < n and W < 64:
        W *= 2
    return W, (1 if n <= W else (2 if n <= 2 * W else 4))


def padded_width(n):
    W, E = library_mapping(n)
    return W * E


def _params(params):
    return np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)


def _solve(fn, objective, m, x0, params, stop, extra):
    x0 = np.ascontiguousarray(x0, dtype=np.float32)
    B, n = x0.shape
    params = _params(params)
    x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B, dtype=np.float32)
    prog = np.zeros(B, dtype=PROGRESS_DTYPE)
    rc = fn(objective, n, m, B, params.ctypes.data, stop.ctypes.data, *extra, x0.ctypes.data, x.ctypes.data,
            f.ctypes.data, g.ctypes.data, prog.ctypes.data)
    assert rc == 0, "unsupported solve"
    return x, f, g, prog


def _declare(fn, n_extra):
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p] + [C.c_int] * n_extra + [C.c_void_p] * 5
    return fn


def _declare_trajectory(fn, n_extra):
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * n_extra + [C.c_void_p] * 5 + \
                  [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


_twin = None


def _twin_lib():
    global _twin
    if _twin is None:
        _twin = C.CDLL(TWIN_LIB)
        _declare(_twin.l32_twin_solve, 2)
        _declare_trajectory(_twin.l32_twin_trajectory, 2)
        _twin.l32_twin_eval.restype = C.c_int
        _twin.l32_twin_eval.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3
    return _twin


def default_stop():
    return make_stop(**STOP_PRESETS["default"])


def twin_solve(objective, m, x0, params=None, stop=None, order=REF_ORDER, width=None):
    """The CPU twin: (x, f, g, progress) of every row of x0 (float32).  width: W x E of the device order."""
    n = np.asarray(x0).shape[1]
    return _solve(_twin_lib().l32_twin_solve, objective, m, x0, params, stop if stop is not None else default_stop(),
                  (order, width if width is not None else padded_width(n)))


def twin_eval(objective, x, params=None, order=DEVICE_ORDER, width=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, n = x.shape
    params = _params(params)
    f, g = np.empty(B, dtype=np.float32), np.empty_like(x)
    rc = _twin_lib().l32_twin_eval(objective, n, B, params.ctypes.data, order,
                                   width if width is not None else padded_width(n), x.ctypes.data, f.ctypes.data,
                                   g.ctypes.data)
    assert rc == 0
    return f, g


def _trajectory(fn, extra, objective, m, x0, params, stop, capacity):
    x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float32).reshape(1, -1))
    n = x0.shape[1]
    params = _params(params)
    stop = stop if stop is not None else default_stop()
    x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(1, dtype=np.float32)
    prog = np.zeros(1, dtype=PROGRESS_DTYPE)
    rows, xs, count = np.zeros((capacity, 6)), np.zeros((capacity, n), dtype=np.float32), C.c_int(0)
    rc = fn(objective, n, m, params.ctypes.data, stop.ctypes.data, *extra, x0.ctypes.data, x.ctypes.data, f.ctypes.data,
            g.ctypes.data, prog.ctypes.data, capacity, rows.ctypes.data, xs.ctypes.data, C.byref(count))
    assert rc == 0, "unsupported solve"
    k = count.value
    return x, f, g, prog, rows[:k].copy(), xs[:k].copy()


def twin_trajectory(objective, m, x0, params=None, stop=None, order=REF_ORDER, width=None, capacity=10001):
    """One twin solve from x0 with its per-iteration rows [K, 6] (num_iterations, status, value, x_delta, f_delta,
    gradient_norm) and iterates [K, n]."""
    n = np.asarray(x0).reshape(1, -1).shape[1]
    return _trajectory(_twin_lib().l32_twin_trajectory, (order, width if width is not None else padded_width(n)),
                       objective, m, x0, params, stop, capacity)


def build_reference(out_dir):
    """Compile the reference harness over the reference tree into out_dir; returns the library path."""
    lib = os.path.join(out_dir, "libl32_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                           "-I" + os.path.join(REPO, "oracle", "eigen_shim"),
                           "-I" + os.path.join(REFERENCE, "include"), "-I" + L32_DIR,
                           os.path.join(L32_DIR, "ref_harness.cpp"), "-o", lib])
    return lib


def reference_solver(lib_path):
    lib = C.CDLL(lib_path)
    fn = _declare(lib.l32_ref_solve, 0)
    tr = _declare_trajectory(lib.l32_ref_trajectory, 0)

    def solve(objective, m, x0, params=None, stop=None):
        return _solve(fn, objective, m, x0, params, stop if stop is not None else default_stop(), ())

    def trajectory(objective, m, x0, params=None, stop=None, capacity=10001):
        return _trajectory(tr, (), objective, m, x0, params, stop, capacity)
    solve.trajectory = trajectory
    return solve
