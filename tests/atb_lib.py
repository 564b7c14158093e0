"""The cases of the ask/tell L-BFGS-B tests (tests/test_gpu_ask_tell_box.py, tests/test_ask_tell_box_cpu.py) and the
helpers they share.  TEST INFRASTRUCTURE: only tests/ imports this module."""
import os

import numpy as np

import at_lib
import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
BOX_DIR = os.path.join(HERE, "ask_tell_box")
B = 131
DIMS = (3, 16, 17, 33, 64)       # mostly padding; E = 1 full; first E = 2; first E = 4; E = 4 full
HISTORIES = (1, 5, 6, 8)         # a shift every iteration; capacity 5 full; capacity 8 partly used; sixteen LU rows
ASK_KINDS = ("clip_start", "trial", "cauchy", "clip_next", "first")
GRADIENT_STATUS = 4


def width(n):
    """P = 16 E: the padded width of the sixteen-lane mapping of the L-BFGS-B kernels"""
    return 16 if n <= 16 else (32 if n <= 32 else 64)


def box_of(objective, n):
    """Rosenbrock: [-1.5, 0.8]^n (the minimiser (1, ..., 1) lies outside: bounds are active at the solution).
    DiagQuadratic: lower = 0.2 on odd coordinates and -1 elsewhere, upper = 1 (half the bounds active at the solution)."""
    if objective == "rosenbrock":
        return np.full(n, -1.5), np.full(n, 0.8)
    return np.where(np.arange(n) % 2 == 1, 0.2, -1.0), np.full(n, 1.0)


def random_rows(lower, upper, seed, spread=0.2):
    """One box per problem: the rows of the shared box moved by up to `spread` (never crossed)"""
    rng = np.random.default_rng(seed)
    n = len(lower)
    lo = lower + spread * rng.uniform(-1.0, 1.0, (B, n))
    hi = upper + spread * rng.uniform(-1.0, 1.0, (B, n))
    return np.ascontiguousarray(lo), np.ascontiguousarray(np.maximum(hi, lo))


def infeasible_starts(n, seed):
    """Rosenbrock starts for the box [-1.5, 0.8]: every third row has coordinates pushed above the upper bound, every
    fifth one below the lower bound; the others lie inside.  Returns (x0, the rows with clip(x0) != x0)."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-1.4, 0.7, (B, n))
    rows = np.arange(B)
    x0[rows % 3 == 0, ::2] += 1.5
    x0[rows % 5 == 0, 1] -= 3.0
    lo, hi = box_of("rosenbrock", n)
    outside = np.any(np.clip(x0, lo, hi) != x0, axis=1)
    return x0, outside


# ---- test 7: the case in which every cut of the iteration is exercised ---------------------------------------------------
EVERY_CUT = dict(n=33, m=5, seed=7007)


def every_cut_case():
    """Rosenbrock n = 33, one box per problem around [-1.5, 0.8]; the first eight problems are pinned (lower == upper: no
    free variable, the Cauchy point is evaluated), every third start lies outside its box (clip-start), and steps that end
    on a bound leave the box by a rounding of x + 1 (smin - x) (clip-next).  Returns (x0, lower rows, upper rows)."""
    n, seed = EVERY_CUT["n"], EVERY_CUT["seed"]
    lo, hi = random_rows(*box_of("rosenbrock", n), seed=seed, spread=0.1)
    lo[:8] = 0.5
    hi[:8] = 0.5
    x0, _ = infeasible_starts(n, seed + 1)
    return x0, lo, hi


# ---- test 10: an objective the library does not have ---------------------------------------------------------------------
TORCH_DIMS = (13, 40)
TORCH_M = 5


def torch_case(n):
    """f_b(x) = sum_i a_i (x_i - c_{b,i})^2, a_i in [0.5, 2], one box per problem, a third of the c outside it: the
    minimiser is clip(c_b, lo_b, hi_b).  Returns (a, c, lo, hi, x0).  The draw is the one tests/test_ask_tell_box_cpu.py
    clears: the reference algorithm alone (the CPU oracle on DiagQuadratic in shifted coordinates) is within
    at_lib.CONTRACT of the closed form on all problems."""
    rng = np.random.default_rng(52000 + n)
    a = rng.uniform(0.5, 2.0, n)
    lo = rng.uniform(-1.0, -0.2, (B, n))
    hi = rng.uniform(0.2, 1.0, (B, n))
    c = rng.uniform(-1.5, 1.5, (B, n))
    x0 = rng.uniform(-0.15, 0.15, (B, n))
    return a, c, lo, hi, x0


def torch_case_stop():
    """the projected-gradient test alone (1e-8, absolute: lbfgsb.h:280-283), under a limit of 500 iterations"""
    return oracle_lib.make_stop(num_iterations=500, x_delta=0.0, f_delta=0.0, gradient_norm=1e-8,
                                gradient_norm_relative=0, past=0)


def torch_case_oracle_error(n):
    """max over the problems of |x - clip(c)| for the reference algorithm alone: the CPU oracle (reference order) on
    DiagQuadratic in the shifted coordinates z = x - c_b, one call per problem"""
    a, c, lo, hi, x0 = torch_case(n)
    worst = 0.0
    for b in range(B):
        z, _, _, prog = oracle_lib.lbfgsb_minimize_batch("diag_quadratic", (x0[b] - c[b])[None, :], m=TORCH_M,
                                                         stop=torch_case_stop(), params=np.concatenate([a, [0.0]]),
                                                         lower=lo[b] - c[b], upper=hi[b] - c[b])
        assert prog["status"][0] == GRADIENT_STATUS, (b, prog["status"][0])
        x = z[0] + c[b]
        worst = max(worst, float(np.max(np.abs(x - np.clip(c[b], lo[b], hi[b])))))
    return worst


def stop_of(**over):
    return at_lib.base_stop(**over)
