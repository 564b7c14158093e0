"""ctypes helpers of the Nelder-Mead tests: the CPU twin (tests/nelder_mead/nm_twin.hpp, built by build() into
tests/nelder_mead/_build/) and, where the reference tree exists, the reference harness compiled into a directory the
caller names (tests/nelder_mead/ref_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NM_DIR = os.path.join(HERE, "nelder_mead")
REPO = os.path.dirname(HERE)
REFERENCE = "/root/reference"
TWIN_LIB = os.path.join(NM_DIR, "_build", "libnm_twin.so")

ROSENBROCK, DIAG_QUADRATIC, L1_QUADRATIC = 0, 1, 100
REF_ORDER, DEVICE_ORDER = 0, 1
VALUE, FIRST = 0, 1

STOP_DTYPE = np.dtype([("num_iterations", "<u8"), ("x_delta", "<f8"), ("x_delta_violations", "<i4"), ("f_delta", "<f8"),
                       ("f_delta_violations", "<i4"), ("f_delta_relative", "<i4"), ("gradient_norm", "<f8"),
                       ("gradient_norm_relative", "<i4"), ("past", "<i4"), ("past_delta", "<f8")], align=True)
CONFIG_FIELDS = ("rho", "xi", "gamma", "sigma", "degenerate_tol", "mode")
CONFIG_DTYPE = np.dtype([(f, "<i4" if f == "mode" else "<f8") for f in CONFIG_FIELDS], align=True)
PROGRESS_DTYPE = np.dtype([("status", "<i4"), ("num_iterations", "<u4"), ("nfev", "<u4"), ("sum_k", "<u4"),
                           ("x_delta", "<f8"), ("f_delta", "<f8"), ("gradient_norm", "<f8")], align=True)
DEFAULT_CONFIG = dict(rho=1.0, xi=20.0, gamma=0.1, sigma=0.5, degenerate_tol=1e-8, mode=VALUE)
# the stopping presets: DefaultStoppingSolverProgress, ConservativeStoppingSolverProgress (progress.h; as
# mi355_lbfgs_default_stop fills them) and the solver's own default, the conservative one with five x_delta strikes
# (nelder_mead.h:87-91)
_DEFAULT = dict(num_iterations=10000, x_delta=1e-9, x_delta_violations=1, f_delta=0.0, f_delta_violations=1,
                f_delta_relative=0, gradient_norm=1e-5, gradient_norm_relative=1, past=3, past_delta=1e-6)
_CONSERVATIVE = {**_DEFAULT, "gradient_norm": 5e-6, "past": 5, "past_delta": 1e-10}
STOP_PRESETS = {
    "default": _DEFAULT,
    "conservative": _CONSERVATIVE,
    "solver": {**_CONSERVATIVE, "x_delta_violations": 5},
}


class Trajectory(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("count", C.c_int32), ("rows", C.c_void_p), ("xs", C.c_void_p)]


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


def _solve(fn, objective, x0, params, stop, config, extra, trajectory, tied):
    """(x, f, g, progress[, tied][, rows, xs]) of every row of x0; the trajectory is that of row 0."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B, n = x0.shape
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    stop = stop if stop is not None else make_stop(**STOP_PRESETS["solver"])
    config = config if config is not None else make_config()
    x, g, f = np.empty_like(x0), np.empty_like(x0), np.empty(B)
    prog = np.zeros(B, dtype=PROGRESS_DTYPE)
    out = [x.ctypes.data, f.ctypes.data, g.ctypes.data, prog.ctypes.data]
    ties = np.zeros(B, dtype=np.int32)
    if tied:
        out.append(ties.ctypes.data)
    traj, rows, xs = None, None, None
    if trajectory:
        rows, xs = np.zeros((trajectory, 6)), np.zeros((trajectory, n))
        traj = Trajectory(trajectory, 0, rows.ctypes.data, xs.ctypes.data)
    rc = fn(objective, n, B, params.ctypes.data, stop.ctypes.data, config.ctypes.data, *extra, x0.ctypes.data, *out,
            C.byref(traj) if traj is not None else None)
    assert rc == 0, "unsupported solve"
    res = [x, f, g, prog]
    if tied:
        res.append(ties.astype(bool))
    if trajectory:
        res += [rows[:traj.count].copy(), xs[:traj.count].copy()]
    return tuple(res)


_twin = None


def twin_solve(objective, x0, params=None, stop=None, config=None, order=REF_ORDER, W=None, trajectory=0):
    """The CPU twin: (x, f, g, progress, tied[, rows, xs]).  W: the padded width of the device order (default: the
    library's mapping).  tied[b]: a ranking of solve b met two values of which neither is below the other."""
    global _twin
    if _twin is None:
        _twin = C.CDLL(TWIN_LIB).nm_twin_solve
        _twin.restype = C.c_int
        _twin.argtypes = [C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 7
    n = np.asarray(x0).shape[1]
    return _solve(_twin, objective, x0, params, stop, config, (order, W if W is not None else padded_width(n)),
                  trajectory, True)


def build_reference(out_dir):
    """Compile the reference harness over the reference tree into out_dir; returns the library path."""
    lib = os.path.join(out_dir, "libnm_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                           "-I" + os.path.join(NM_DIR, "overlay"), "-I" + os.path.join(REPO, "oracle", "eigen_shim"),
                           "-I" + os.path.join(REFERENCE, "include"), "-I" + NM_DIR,
                           os.path.join(NM_DIR, "ref_harness.cpp"), "-o", lib])
    return lib


def reference_solver(lib_path):
    fn = C.CDLL(lib_path).nm_ref_solve
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 3 + [C.c_void_p] * 6

    def solve(objective, x0, params=None, stop=None, config=None, trajectory=0):
        return _solve(fn, objective, x0, params, stop, config, (), trajectory, False)
    return solve
