"""ctypes helpers of the Newton-descent tests: the CPU twin (tests/newton_descent/nd_twin.hpp, built by build() into
tests/newton_descent/_build/) and, where the reference tree exists, the reference harness compiled into a directory the
caller names (tests/newton_descent/ref_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ND_DIR = os.path.join(HERE, "newton_descent")
REPO = os.path.dirname(HERE)
REFERENCE = "/root/reference"
TWIN_LIB = os.path.join(ND_DIR, "_build", "libnd_twin.so")

ROSENBROCK, DIAG_QUADRATIC, QUARTIC, DENSE = 0, 1, 100, 101
REF_ORDER, DEVICE_ORDER = 0, 1

STOP_DTYPE = np.dtype([("num_iterations", "<u8"), ("x_delta", "<f8"), ("x_delta_violations", "<i4"), ("f_delta", "<f8"),
                       ("f_delta_violations", "<i4"), ("f_delta_relative", "<i4"), ("gradient_norm", "<f8"),
                       ("gradient_norm_relative", "<i4"), ("past", "<i4"), ("past_delta", "<f8")], align=True)
CONFIG_FIELDS = ("safe_guard", "armijo_c", "armijo_rho")
CONFIG_DTYPE = np.dtype([(f, "<f8") for f in CONFIG_FIELDS], align=True)
PROGRESS_DTYPE = np.dtype([("status", "<i4"), ("num_iterations", "<u4"), ("nfev", "<u4"), ("sum_k", "<u4"),
                           ("x_delta", "<f8"), ("f_delta", "<f8"), ("gradient_norm", "<f8")], align=True)
COUNTERS_DTYPE = np.dtype([("interchanges", "<u4"), ("max_trials", "<u4"), ("alpha_one_steps", "<u4"),
                           ("alpha_less_steps", "<u4"), ("fixed_point", "<u4"), ("pivot_ties", "<u4"),
                           ("zero_columns", "<u4"), ("conditions", "<u4"), ("pivot_distance", "<u4", (64,)),
                           ("min_condition_margin", "<f8")], align=True)
NO_MUTATION, TRANSPOSE_BEFORE_LU, CHAIN_WALKS_ROW = 0, 1, 2    # nd_twin::Mutation
DEFAULT_CONFIG = dict(safe_guard=1e-5, armijo_c=0.2, armijo_rho=0.9)   # newton_descent.h:69, armijo.h:85-86
# the stopping presets: DefaultStoppingSolverProgress (progress.h; as mi355_lbfgs_default_stop fills it) and the
# package's parity preset (cppnumericalsolvers_amd.parity_stop)
_DEFAULT = dict(num_iterations=10000, x_delta=1e-9, x_delta_violations=1, f_delta=0.0, f_delta_violations=1,
                f_delta_relative=0, gradient_norm=1e-5, gradient_norm_relative=1, past=3, past_delta=1e-6)
STOP_PRESETS = {
    "default": _DEFAULT,
    "parity": {**_DEFAULT, "x_delta": 1e-11, "gradient_norm": 1e-8, "past": 0},
}
# alpha *= 0.9 from 1 stops changing after this many multiplications (alpha = 2.5e-323): the bound of the search
FIXED_POINT_SHRINKS = 7050


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


def padded_width(n):
    W = 8
    while W < n:
        W *= 2
    return W


def _solve(fn, objective, x0, params, stop, config, condition_stop, extra, counters=False):
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B, n = x0.shape
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B)
    prog = np.zeros(B, dtype=PROGRESS_DTYPE)
    tail = []
    if counters:
        cnt = np.zeros(B, dtype=COUNTERS_DTYPE)
        tail = [cnt.ctypes.data]
    rc = fn(objective, n, B, params.ctypes.data, stop.ctypes.data, C.c_double(condition_stop), config.ctypes.data,
            *extra, x0.ctypes.data, x.ctypes.data, f.ctypes.data, g.ctypes.data, prog.ctypes.data, *tail)
    assert rc == 0, "unsupported solve"
    return (x, f, g, prog, cnt) if counters else (x, f, g, prog)


def _declare(fn, n_extra, n_tail):
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p] + [C.c_int] * n_extra + \
                  [C.c_void_p] * (5 + n_tail)
    return fn


_twin = None


def _twin_lib():
    global _twin
    if _twin is None:
        _twin = C.CDLL(TWIN_LIB)
        _declare(_twin.nd_twin_solve, 2, 1)
        _declare(_twin.nd_twin_solve_mutated, 3, 0)
        _twin.nd_twin_lu_factor.restype = C.c_int
        _twin.nd_twin_lu_factor.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _twin.nd_twin_lu_solve.restype = C.c_int
        _twin.nd_twin_lu_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _twin.nd_twin_condition.restype = C.c_double
        _twin.nd_twin_condition.argtypes = [C.c_void_p, C.c_int]
        _twin.nd_twin_search.restype = C.c_int
        _twin.nd_twin_search.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    return _twin


def twin_solve(objective, x0, params=None, stop=None, config=None, condition_stop=0.0, order=REF_ORDER, W=None,
               counters=False):
    """The CPU twin: (x, f, g, progress[, counters]) of every row of x0.  W: the padded width of the device order
    (default: the library's mapping, the next power of two >= max(n, 8))."""
    n = np.asarray(x0).shape[1]
    out = _solve(_twin_lib().nd_twin_solve, objective, x0, params,
                 stop if stop is not None else make_stop(**STOP_PRESETS["default"]),
                 config if config is not None else make_config(), condition_stop,
                 (order, W if W is not None else padded_width(n)), counters=True)
    return out if counters else out[:4]


def twin_solve_mutated(mutation, objective, x0, params=None, stop=None, config=None, condition_stop=0.0, order=REF_ORDER,
                       W=None):
    """twin_solve with one of the twin's deliberate bugs planted (TRANSPOSE_BEFORE_LU, CHAIN_WALKS_ROW)."""
    n = np.asarray(x0).shape[1]
    return _solve(_twin_lib().nd_twin_solve_mutated, objective, x0, params,
                  stop if stop is not None else make_stop(**STOP_PRESETS["default"]),
                  config if config is not None else make_config(), condition_stop,
                  (order, W if W is not None else padded_width(n), mutation))


def _column_major(A):
    A = np.asarray(A, dtype=np.float64)
    assert A.ndim == 2 and A.shape[0] == A.shape[1]
    return np.ascontiguousarray(A.T).reshape(-1).copy()


def twin_lu(A):
    """The twin's LU of A ([n, n], A[i, j] = A(i, j)): (LU [n, n] with the unit-lower multipliers below the diagonal,
    piv: row piv[k] was exchanged with row k at step k)."""
    n = A.shape[0]
    a, piv = _column_major(A), np.zeros(n, dtype=np.int32)
    assert _twin_lib().nd_twin_lu_factor(a.ctypes.data, piv.ctypes.data, n) == 0
    return a.reshape(n, n).T.copy(), piv


def twin_lu_solve(LU, piv, b):
    """x of A x = b through the twin's substitutions on the factors of twin_lu."""
    n = LU.shape[0]
    a, x = _column_major(LU), np.array(b, dtype=np.float64)
    piv = np.ascontiguousarray(piv, dtype=np.int32)
    assert _twin_lib().nd_twin_lu_solve(a.ctypes.data, piv.ctypes.data, x.ctypes.data, n) == 0
    return x


def twin_condition(A):
    """The twin's ||A||_F ||A^-1||_F."""
    a = _column_major(A)
    return _twin_lib().nd_twin_condition(a.ctypes.data, A.shape[0])


def twin_search(objective, x, d, params=None, config=None, order=REF_ORDER, W=None):
    """One Armijo search of the twin from x along d: (alpha, trial points, ended at the fixed point of alpha *= rho)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    n = x.shape[0]
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    config = config if config is not None else make_config()
    alpha, trials, fixed = C.c_double(0), C.c_uint32(0), C.c_int32(0)
    rc = _twin_lib().nd_twin_search(objective, n, params.ctypes.data, config.ctypes.data, order,
                                    W if W is not None else padded_width(n), x.ctypes.data, d.ctypes.data,
                                    C.addressof(alpha), C.addressof(trials), C.addressof(fixed))
    assert rc == 0
    return alpha.value, trials.value, bool(fixed.value)


def build_reference(out_dir):
    """Compile the reference harness over the reference tree into out_dir; returns the library path.  (The Eigen
    stand-in covers everything newton_descent.h and armijo.h use — scalar * row vector, row vector * matrix, the 1 x 1
    product added to a scalar — each an ascending sum: no overlay is needed.)"""
    lib = os.path.join(out_dir, "libnd_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                           "-I" + os.path.join(REPO, "oracle", "eigen_shim"),
                           "-I" + os.path.join(REFERENCE, "include"), "-I" + ND_DIR,
                           os.path.join(ND_DIR, "ref_harness.cpp"), "-o", lib])
    return lib


def reference_trajectory(lib_path, objective, x0, params=None, stop=None, config=None, condition_stop=0.0,
                         capacity=1000):
    """One reference solve from x0 (a single start) with its per-iteration states from the reference's step callback:
    (x, f, g, progress, rows [K, 6] = num_iterations, status, value, x_delta, f_delta, gradient_norm, xs [K, n])."""
    fn = C.CDLL(lib_path).nd_ref_trajectory
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
    fn = _declare(C.CDLL(lib_path).nd_ref_solve, 0, 0)

    def solve(objective, x0, params=None, stop=None, config=None, condition_stop=0.0):
        return _solve(fn, objective, x0, params, stop if stop is not None else make_stop(**STOP_PRESETS["default"]),
                      config if config is not None else make_config(), condition_stop, ())
    return solve


def twin_solve_threaded(objective, x0, params=None, stop=None, config=None, condition_stop=0.0, order=REF_ORDER, W=None,
                        threads=8):
    """twin_solve over chunks of rows on `threads` host threads (the C call releases the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B = x0.shape[0]
    _twin_lib()
    bounds = np.linspace(0, B, 4 * threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda i: twin_solve(objective, x0[bounds[i]:bounds[i + 1]], params, stop, config,
                                                   condition_stop, order=order, W=W), range(4 * threads)))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
