"""Batches of the work-queue tests (tests/test_gpu_work_queue.py): mixed start points that give a persistent kernel
problems of very different lengths back to back, with degenerate rows spliced in, and a threaded front of the CPU
twin (the twin solves every row on its own, so chunks of rows may run side by side)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import tr_lib as T

SCALES = (0.05, 0.5, 2.0, 3.0)
FIELDS = ("status", "num_iterations", "nfev", "sum_k", "x_delta", "f_delta", "gradient_norm")


def padded_width(n):
    W = 8
    while W < n:
        W *= 2
    return W


def mixed_starts(n, B, seed):
    """x0 = 1 + s u, s drawn per row from SCALES, u uniform in [-1, 1]: Rosenbrock solves of 5 to 250 iterations."""
    rng = np.random.default_rng(seed)
    s = rng.choice(SCALES, size=B)
    return 1.0 + s[:, None] * rng.uniform(-1.0, 1.0, (B, n))


def spliced_rows(B):
    """(rows of exact ones, rows of 1e100): positions spread over the batch, the first and the last row among them, never
    two of them neighbours."""
    ones = sorted({0, B // 9 + 1, (3 * B) // 9, (5 * B) // 9 + 1, (7 * B) // 9})
    big = sorted({(2 * B) // 9, (4 * B) // 9 + 1, (6 * B) // 9, (8 * B) // 9 + 1, B - 1})
    assert not set(ones) & set(big)
    return np.array(ones), np.array(big)


def mixed_rosenbrock_batch(n, B, seed):
    """(x0, rows of ones, rows of 1e100).  A row of ones stalls at the minimiser (the in-step rejection loop runs dry);
    a row of 1e100 overflows f and takes the NaN-rho retry path."""
    x0 = mixed_starts(n, B, seed)
    ones, big = spliced_rows(B)
    x0[ones] = 1.0
    x0[big] = 1e100
    return x0, ones, big


def twin_solve(objective, x0, params=None, stop=None, config=None, condition_stop=0.0, order=T.REF_ORDER, W=None,
               threads=8):
    """tr_lib.twin_solve over chunks of rows on `threads` host threads (the C call releases the interpreter lock)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    B = x0.shape[0]
    if B < 4 * threads:
        return T.twin_solve(objective, x0, params, stop, config, condition_stop, order=order, W=W)
    T.twin_solve(objective, x0[:1], params, stop, config, condition_stop, order=order, W=W)   # (loads the library once)
    bounds = np.linspace(0, B, 4 * threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda i: T.twin_solve(objective, x0[bounds[i]:bounds[i + 1]], params, stop, config,
                                                     condition_stop, order=order, W=W), range(4 * threads)))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def same_bits(a, b):
    """Every array of (x, f, g) and every progress field equal byte for byte; returns the first difference or None."""
    for name, u, v in zip(("x", "f", "g"), a[:3], b[:3]):
        if u.tobytes() != v.tobytes():
            rows = np.nonzero((u.view(np.uint64) != v.view(np.uint64)).reshape(u.shape[0], -1).any(axis=1))[0]
            return "%s differs in %d rows, first %d" % (name, rows.size, rows[0])
    for k in FIELDS:
        u, v = np.ascontiguousarray(a[3][k]), np.ascontiguousarray(b[3][k])
        if u.tobytes() != v.tobytes():
            rows = np.nonzero((u.view(np.uint8).reshape(len(u), -1) != v.view(np.uint8).reshape(len(v), -1)).any(axis=1))[0]
            return "progress.%s differs in %d rows, first %d: %r != %r" % (k, rows.size, rows[0], u[rows[0]], v[rows[0]])
    return None
