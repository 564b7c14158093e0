"""Inputs and rows of the L-BFGS-B step audit (tests/bstep_lib.py): tests/test_bstep_lib.py runs them on the CPU twins,
tests/test_gpu_lbfgsb_steps_mpmath.py on the device.

Batches of 24 with the 8 traced problems of tests/step_cases.py.  Stop record: an iteration limit of 3 m + 8, `f_delta` off
(the reference's default f_delta test is no part of the step), the projected-gradient test at 1e-6 so that a run ends before
the rounding regime; every other test off.

The inputs are chosen so that the step's branches run WITH history (tests/test_bstep_lib.py asserts the counts on the
reference-order twin).  In the box of tests/step_cases.py every breakpoint crossing falls in iteration 0, where W is empty.
  diag_quadratic   sum a_j x_j^2 + c, a from 1e-2 to 1 (spread 1e2), in [0.5, 2] (one box per problem: [0.1, 1] moved by up to 0.02): the centre lies outside the lower faces, the
                   minimiser is the corner, and the coordinates reach their bounds one group after another — breakpoints are
                   crossed with pairs stored, and the last steps have no free variable.
  rosenbrock       shared box [1.5, 2]: the minimiser is the corner (lo, .., lo, hi).  One box per problem: [0.2, 0.6],
                   [1.5, 2], [0.5, 0.6] in turn, each moved by up to 0.02: a minimiser cut off on some sides only, a corner,
                   and a thin box.
Starts are uniform in the box; every other problem has its first two coordinates ON a bound (t_j = 0).
"""
import numpy as np

import step_cases as Sc
import step_lib

B = Sc.B
TRACED = Sc.TRACED
GRADIENT_NORM = 1e-6
limit = Sc.limit
ROSENBROCK_BOXES = ((0.2, 0.6), (1.5, 2.0), (0.5, 0.6))


def stop_fields(num_iterations, gradient_norm=GRADIENT_NORM):
    return dict(num_iterations=num_iterations, x_delta=0.0, x_delta_violations=1, f_delta=0.0, f_delta_violations=1,
                f_delta_relative=0, gradient_norm=gradient_norm, gradient_norm_relative=0, past=0, past_delta=0.0)


def coefficients(n):
    return (np.geomspace(1e-2, 1.0, n) if n > 1 else np.ones(1)), 0.25


def blob(name, n):
    if name == "rosenbrock":
        return None
    a, c = coefficients(n)
    return np.concatenate([a, [c]])


def boxes(name, n, own):
    """lower, upper [B, n]"""
    rng = np.random.default_rng(1000 + n)
    shift = 0.02 * rng.uniform(0.0, 1.0, (B, 1)) if own else np.zeros((B, 1))
    if name == "rosenbrock":
        pick = [ROSENBROCK_BOXES[b % 3] if own else ROSENBROCK_BOXES[1] for b in range(B)]
    else:
        pick = [(0.1, 1.0) if own else (0.5, 2.0)] * B
    lower = np.array([[lo] * n for lo, _ in pick]) + shift
    upper = np.array([[hi] * n for _, hi in pick]) + shift
    return lower, upper


def starts(name, n, m, lower, upper):
    rng = np.random.default_rng(100 * n + m)
    x0 = lower + (upper - lower) * rng.uniform(0.0, 1.0, (B, n))
    x0[::2, 0] = lower[::2, 0]
    x0[::2, 1 % n] = upper[::2, 1 % n]
    return x0


def case(name, n, m, own):
    lower, upper = boxes(name, n, own)
    return blob(name, n), lower, upper, starts(name, n, m, lower, upper)


def rules(family, m, lower, upper, linesearch="more_thuente"):
    """the depth of an inner product: the reference's sums are sequential, the kernels' are trees, the relaxed kernel's a
    fused chain per lane"""
    dot = {"reference": "sequential", "relaxed": "fused"}.get(family, "tree")
    return step_lib.Rules(m, solver="lbfgsb", dot=dot, lower=lower, upper=upper, linesearch=linesearch)


# ---- rows: (objective, n, m, one box per problem) ---------------------------------------------------------------------------------
# (n = 2: two breakpoints crossed leave no free variable, (b) cannot occur; and no n = 2 input found has (c) next to (a): the
# Rosenbrock boxes give alpha* < 1 but cross their breakpoints in iteration 0, the quadratic crosses them with history but its
# subspace step stays inside.  That row is held to (a), (d), (e).)
CPU_ROWS = (("diag_quadratic", 2, 1, True), ("rosenbrock", 7, 3, True), ("rosenbrock", 8, 1, True),
            ("rosenbrock", 9, 3, False), ("diag_quadratic", 9, 3, True), ("rosenbrock", 17, 5, True),
            ("diag_quadratic", 17, 8, False), ("rosenbrock", 33, 5, True), ("rosenbrock", 33, 10, False),
            ("diag_quadratic", 33, 10, False), ("diag_quadratic", 64, 3, False), ("rosenbrock", 64, 8, False),
            ("rosenbrock", 64, 8, True), ("diag_quadratic", 17, 10, False))
# eight coordinates per lane on the device: three traced problems
E8_TRACED = TRACED[:3]
E8_ROWS = (("rosenbrock", 100, 3, False), ("diag_quadratic", 200, 3, False))
# (a row on which the Hager-Zhang search takes another path than More-Thuente: 3 of its 8 problems)
HZ_ROW = ("rosenbrock", 17, 5, True)
# the generator's rows (no twin: the planted bugs)
GENERATOR_ROWS = (("diag_quadratic", 7, 3, False), ("rosenbrock", 9, 3, True), ("diag_quadratic", 17, 5, False),
                  ("rosenbrock", 17, 5, False), ("rosenbrock", 33, 5, True), ("diag_quadratic", 33, 8, False),
                  ("rosenbrock", 8, 1, True), ("diag_quadratic", 9, 3, True))


def prefix_trajectories(solve, x0, f0, g0, m):
    """tests/step_cases.py's, under this module's stop record"""
    return Sc.prefix_trajectories(solve, x0, f0, g0, m, fields=stop_fields, first_fields=lambda: stop_fields(1, 1e300))
