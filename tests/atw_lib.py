"""ctypes binding of the CPU twin of the ask/tell L-BFGS kernel above n = 256 (tests/ask_tell_wide/_build/libatw_twin.so),
the cases of its tests and the driver loops they share.  TEST INFRASTRUCTURE: only tests/ imports this module.  The
comparison helpers, the start points and the stop records are tests/at_lib.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

import at_lib
import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
TWIN_DIR = os.path.join(HERE, "ask_tell_wide")
LIB_PATH = os.path.join(TWIN_DIR, "_build", "libatw_twin.so")
HEADER_TEST = os.path.join(TWIN_DIR, "_build", "atw_header_test")
BIG_N = 32768   # kWideBigN: 1024 threads per problem from here on

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", TWIN_DIR, LIB_PATH])
        L = C.CDLL(LIB_PATH)
        dp = C.POINTER(C.c_double)
        L.atw_create.argtypes = [C.c_int, C.c_int, C.POINTER(oracle_lib.Stop), C.c_int, C.c_int64, dp]
        L.atw_create.restype = C.c_void_p
        L.atw_x.argtypes = [C.c_void_p]
        L.atw_x.restype = dp
        L.atw_tell.argtypes = [C.c_void_p, dp, dp]
        L.atw_tell.restype = C.c_int64
        L.atw_results.argtypes = [C.c_void_p, dp, dp, dp, C.c_void_p]
        L.atw_results.restype = None
        L.atw_drive.argtypes = [C.c_void_p, C.c_int, dp, C.c_int64]
        L.atw_drive.restype = C.c_int64
        L.atw_eval.argtypes = [C.c_int, dp, C.c_int, C.c_int, dp, dp]
        L.atw_eval.restype = C.c_double
        L.atw_destroy.argtypes = [C.c_void_p]
        L.atw_destroy.restype = None
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def threads(n):
    """T: the threads a problem's workgroup has, hence the lanes of the strided summation order"""
    return 1024 if n >= BIG_N else 256


class Twin:
    """One solve of the twin stepper: `.x` is a numpy view of its evaluation buffer, tell(f, g) -> active."""

    def __init__(self, x0, m, stop, width=None):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        self.B, self.n = x0.shape
        self._stop = stop
        self._h = lib().atw_create(self.n, int(m), C.byref(stop), int(width or threads(self.n)), self.B, _dp(x0))
        if not self._h:
            raise ValueError("atw_create refused its arguments")
        self.x = np.ctypeslib.as_array(lib().atw_x(self._h), shape=(self.B, self.n))

    def tell(self, f, g):
        f = np.ascontiguousarray(f, dtype=np.float64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        assert f.shape == (self.B,) and g.shape == (self.B, self.n)
        return int(lib().atw_tell(self._h, _dp(f), _dp(g)))

    def results(self):
        x, g = np.empty((self.B, self.n)), np.empty((self.B, self.n))
        f = np.empty(self.B)
        prog = np.zeros(self.B, dtype=oracle_lib.PROGRESS_DTYPE)
        lib().atw_results(self._h, _dp(x), _dp(f), _dp(g), prog.ctypes.data)
        return x, f, g, prog

    def drive(self, objective, params=None, max_rounds=1000000):
        """the whole loop in C++ with the oracle's functor in the twin's own order; returns the rounds"""
        p = np.ascontiguousarray(params, dtype=np.float64) if params is not None else None
        rounds = int(lib().atw_drive(self._h, oracle_lib.OBJ[objective], _dp(p) if p is not None else None, max_rounds))
        assert rounds >= 0, "atw_drive did not finish the batch"
        return rounds

    def close(self):
        if self._h:
            lib().atw_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def evaluate(objective, X, params=None, width=None):
    """(f [B], g [B, n]) of the oracle's functor on every row of X in the strided order of `width` lanes (default: the
    kernel's threads at this n) — the evaluation oracle.minimize_batch(reduction="strided", width=T) runs.  Not
    oracle_lib.evaluate(reduction="strided"): oracle_eval knows the sequential and the butterfly order only and, asked
    for "strided", sums the first `width` terms in butterfly order (right up to n = width + 1 for Rosenbrock, n = width
    for DiagQuadratic, and no further)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    B, n = X.shape
    p = np.ascontiguousarray(params, dtype=np.float64) if params is not None else None
    f, g = np.empty(B), np.empty_like(X)
    for b in range(B):
        f[b] = lib().atw_eval(oracle_lib.OBJ[objective], _dp(p) if p is not None else None, n, int(width or threads(n)),
                              _dp(X[b]), _dp(g[b]))
    return f, g


def oracle_callback(objective, params, width):
    """fn(X) -> (f, g): the oracle's functor row by row in the strided order of `width` lanes"""
    return lambda X: evaluate(objective, X, params=params, width=width)


def twin_minimize(objective, x0, m, stop, params=None, poison_finished=None):
    """(x, f, g, progress, rounds) of the twin stepper fed oracle_lib.evaluate (at_lib.drive is the loop)"""
    width = threads(np.asarray(x0).shape[1])
    t = Twin(x0, m, stop, width)
    try:
        rounds = at_lib.drive(t, oracle_callback(objective, params, width), poison_finished=poison_finished)
        return t.results() + (rounds,)
    finally:
        t.close()


def twin_minimize_driven(objective, x0, m, stop, params=None):
    t = Twin(x0, m, stop)
    try:
        rounds = t.drive(objective, params)
        return t.results() + (rounds,)
    finally:
        t.close()


def oracle_minimize(objective, x0, m, stop, params=None):
    """oracle.minimize_batch in the strided order of the kernel's threads: the persistent wide kernel's twin"""
    return oracle_lib.minimize_batch(objective, x0, m=m, stop=stop, params=params, reduction="strided",
                                     width=threads(np.asarray(x0).shape[1]))


# ---- cases -------------------------------------------------------------------------------------------------------------
# (objective, n, m, B)
TWIN_CASES = (("rosenbrock", 257, 6, 9), ("rosenbrock", 300, 10, 12), ("diag_quadratic", 513, 17, 8),
              ("diag_quadratic", 700, 6, 9))
MAX_ITERATIONS = 120


def stops():
    """{name: stop}: the default, parity and conservative records under an iteration limit that keeps a case short"""
    default = oracle_lib.default_stop()
    default.num_iterations = MAX_ITERATIONS
    conservative = oracle_lib.default_stop("conservative")
    conservative.num_iterations = MAX_ITERATIONS
    return {"default": default, "parity": at_lib.base_stop(num_iterations=MAX_ITERATIONS), "conservative": conservative}


# the torch objective of tests/test_gpu_ask_tell_wide.py (test 8): fn(X) = (a * X * X).sum(1) + c, a in [0.5, 20]
TORCH_DIMS = (300, 1000)
TORCH_B = 33
TORCH_C = 0.25
GRADIENT_STATUS = 4


def torch_case(n):
    """(a [n], x0 [B, n]) and the stop: the gradient test alone, relative, 1e-8, under a limit of 1000"""
    rng = np.random.default_rng(7300 + n)
    a = rng.uniform(0.5, 20.0, n)
    x0 = rng.uniform(-2.0, 2.0, (TORCH_B, n))
    return a, x0


def torch_case_stop():
    return oracle_lib.make_stop(num_iterations=1000, x_delta=0.0, f_delta=0.0, gradient_norm=1e-8,
                                gradient_norm_relative=1, past=0)
