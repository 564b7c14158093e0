"""ctypes binding of the CPU twin of the ask/tell L-BFGS kernel (tests/ask_tell/_build/libat_twin.so), the cases of the
ask/tell tests and the driver loops they share.  TEST INFRASTRUCTURE: only tests/ imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
TWIN_DIR = os.path.join(HERE, "ask_tell")
LIB_PATH = os.path.join(TWIN_DIR, "_build", "libat_twin.so")
PROGRESS_FIELDS = ("status", "num_iterations", "nfev", "sum_k", "x_delta", "f_delta", "gradient_norm")
SEQUENTIAL, BUTTERFLY = 0, 1

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", TWIN_DIR, LIB_PATH])
        L = C.CDLL(LIB_PATH)
        dp = C.POINTER(C.c_double)
        L.at_create.argtypes = [C.c_int, C.c_int, C.POINTER(oracle_lib.Stop), C.c_int, C.c_int, C.c_int64, dp]
        L.at_create.restype = C.c_void_p
        L.at_x.argtypes = [C.c_void_p]
        L.at_x.restype = dp
        L.at_tell.argtypes = [C.c_void_p, dp, dp]
        L.at_tell.restype = C.c_int64
        L.at_results.argtypes = [C.c_void_p, dp, dp, dp, C.c_void_p]
        L.at_results.restype = None
        L.at_drive.argtypes = [C.c_void_p, C.c_int, dp, C.c_int64]
        L.at_drive.restype = C.c_int64
        L.at_destroy.argtypes = [C.c_void_p]
        L.at_destroy.restype = None
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def padded_width(n):
    """P = lanes x coordinates per lane of the library's own mapping of n: the padded width up to 64, then 128, 256"""
    P = 8
    while P < n:
        P <<= 1
    return P


class Twin:
    """One solve of the twin stepper: `.x` is a numpy view of its evaluation buffer, tell(f, g) -> active."""

    def __init__(self, x0, m, stop, order=SEQUENTIAL, width=None):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        self.B, self.n = x0.shape
        self._stop = stop
        self._h = lib().at_create(self.n, int(m), C.byref(stop), int(order), int(width or padded_width(self.n)), self.B,
                                  _dp(x0))
        if not self._h:
            raise ValueError("at_create refused its arguments")
        self.x = np.ctypeslib.as_array(lib().at_x(self._h), shape=(self.B, self.n))

    def tell(self, f, g):
        f = np.ascontiguousarray(f, dtype=np.float64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        assert f.shape == (self.B,) and g.shape == (self.B, self.n)
        return int(lib().at_tell(self._h, _dp(f), _dp(g)))

    def results(self):
        x, g = np.empty((self.B, self.n)), np.empty((self.B, self.n))
        f = np.empty(self.B)
        prog = np.zeros(self.B, dtype=oracle_lib.PROGRESS_DTYPE)
        lib().at_results(self._h, _dp(x), _dp(f), _dp(g), prog.ctypes.data)
        return x, f, g, prog

    def close(self):
        if self._h:
            lib().at_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def oracle_callback(objective, params, order, width):
    """fn(X) -> (f, g): oracle_lib.evaluate row by row, in the summation order of the twin it feeds"""
    reduction = "butterfly" if order == BUTTERFLY else "sequential"

    def fn(X):
        f, g = np.empty(X.shape[0]), np.empty_like(X)
        for b in range(X.shape[0]):
            f[b], g[b] = oracle_lib.evaluate(objective, X[b], params=params, reduction=reduction, width=width)
        return f, g
    return fn


def drive(twin, fn, max_rounds=100000, poison_finished=None):
    """The ask/tell loop; poison_finished: a value written over the f / g rows of problems that had finished before the
    round (their rows are never read).  Returns the number of rounds."""
    done = np.zeros(twin.B, dtype=bool)
    rounds, active = 0, twin.B
    while active > 0:
        assert rounds < max_rounds, "the batch did not finish"
        f, g = fn(twin.x.copy())
        if poison_finished is not None:
            f[done] = poison_finished
            g[done] = poison_finished
        active = twin.tell(f, g)
        rounds += 1
        done = _finished(twin)
        assert active == int(np.count_nonzero(~done))
    return rounds


def _finished(twin):
    return twin.results()[3]["status"] > 0


def twin_minimize(objective, x0, m, stop, params=None, order=SEQUENTIAL, width=None, poison_finished=None):
    """(x, f, g, progress, rounds) of the twin stepper fed the oracle's evaluations"""
    width = width or padded_width(np.asarray(x0).shape[1])
    t = Twin(x0, m, stop, order, width)
    try:
        rounds = drive(t, oracle_callback(objective, params, order, width), poison_finished=poison_finished)
        return t.results() + (rounds,)
    finally:
        t.close()


def twin_minimize_driven(objective, x0, m, stop, params=None, order=BUTTERFLY, width=None, max_rounds=1000000):
    """The same through the twin's own loop (at_drive: the oracle's functors evaluated in C++), for the batches of the
    GPU tests"""
    width = width or padded_width(np.asarray(x0).shape[1])
    t = Twin(x0, m, stop, order, width)
    try:
        p = np.ascontiguousarray(params, dtype=np.float64) if params is not None else None
        rounds = int(lib().at_drive(t._h, oracle_lib.OBJ[objective], _dp(p) if p is not None else None, max_rounds))
        assert rounds >= 0, "at_drive did not finish the batch"
        return t.results() + (rounds,)
    finally:
        t.close()


def same_bits(a, b, nan_equal=False):
    """bit for bit; nan_equal: a NaN equals a NaN whatever its sign and payload (they are the processor's: the device's
    and the host's differ)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return np.zeros(a.shape, dtype=bool)
    same = a.view(np.uint64) == b.view(np.uint64)
    return same | (np.isnan(a) & np.isnan(b)) if nan_equal else same


def assert_same_results(got, want, what="", nan_equal=False):
    """x, f, g bit for bit and every progress field, on every problem"""
    B = len(want[1])
    for name, a, b in zip(("x", "f", "g"), got[:3], want[:3]):
        same = same_bits(a, b, nan_equal)
        if not (same.shape == np.shape(b) and same.all()):
            bad = np.nonzero(~same.reshape(B, -1).all(axis=1))[0]
            raise AssertionError("%s: %s differs on %d problems, first %s" % (what, name, len(bad), bad[:8].tolist()))
    for field in PROGRESS_FIELDS:
        a, b = np.asarray(got[3][field]), np.asarray(want[3][field])
        same = same_bits(a, b, nan_equal) if a.dtype == np.float64 else (a == b)
        if not same.all():
            bad = np.nonzero(~same)[0]
            raise AssertionError("%s: progress.%s differs on %d problems, first %s: %s vs %s"
                                 % (what, field, len(bad), bad[:8].tolist(), a[bad[:4]], b[bad[:4]]))


# ---- cases -------------------------------------------------------------------------------------------------------------
DIMS = (2, 5, 8, 13, 33, 64, 65, 130)
HISTORIES = (1, 3, 6, 10)
MAX_ITERATIONS = 200


def diag_params(n):
    """a_i spread over [0.5, 50], c = 0.25"""
    return np.concatenate([0.5 + 49.5 * np.arange(n) / max(n - 1, 1), [0.25]])


def starts(objective, B, n, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    if objective == "rosenbrock":
        base = np.where(np.arange(n) % 2 == 0, -1.2, 1.0)
        return base + spread * rng.uniform(-1.0, 1.0, (B, n))
    return rng.uniform(-2.0, 2.0, (B, n))


def base_stop(**over):
    """the parity stop under an iteration limit that keeps a case short"""
    return oracle_lib.make_stop(**{**dict(num_iterations=MAX_ITERATIONS, x_delta=1e-11, x_delta_violations=1, f_delta=0.0,
                                          gradient_norm=1e-8, gradient_norm_relative=1, past=0), **over})


def stop_records():
    """{name: stop}: the stopping records of tests/stop_cases.py (the first-order table) over the default preset under
    the iteration limit of these tests; one has past > 0 and one ends on the iteration limit."""
    import stop_cases
    out = {}
    for name, (over, _target) in stop_cases.edges("gd").items():
        over = dict(over)
        if over.get("num_iterations", 1) == 0:
            continue   # (no limit: a case of these tests stays bounded)
        out[name] = oracle_lib.make_stop(**{**dict(num_iterations=MAX_ITERATIONS), **over})
    return out


def params_of(objective, n):
    return diag_params(n) if objective == "diag_quadratic" else None


# the inputs of the GPU test's torch-objective comparison (test 3 of tests/test_gpu_ask_tell.py): cleared by
# tests/test_ask_tell_twin.py (cross-order gap <= CONTRACT, status agreement)
CONTRACT = 1e-6
TORCH_CASES = (("rosenbrock", 8, 6), ("rosenbrock", 33, 6), ("diag_quadratic", 13, 3), ("diag_quadratic", 65, 10))
TORCH_B = 131
MAX_STATUS_DISAGREEMENT = 0.02


def torch_case_inputs(objective, n):
    """Rosenbrock starts within 0.05 of the classic one: from the 0.3 spread of the other tests a tenth of the n = 33
    batch stalls at its noise floor once the x_delta test is off and runs 16 trials per iteration to the limit"""
    return starts(objective, TORCH_B, n, seed=4100 + n, spread=0.05)


def torch_case_stop():
    """The gradient test alone (under an iteration limit).  Under the parity record the x_delta and the gradient test
    race on Rosenbrock and the summation order decides which fires first (half the statuses of the n = 33 batch differ
    between the twin's two orders); with one test live the status does not hang on the rounding."""
    return oracle_lib.make_stop(num_iterations=1000, x_delta=0.0, f_delta=0.0, gradient_norm=1e-8,
                                gradient_norm_relative=1, past=0)
