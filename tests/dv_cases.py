"""The case table of the derivative-checker tests (tests/test_derivatives_twin.py, tests/test_gpu_derivatives.py).

Inputs are drawn here from fixed seeds; tests/golden/derivatives_reference_vectors.npz (tests/golden/make_golden_dv.py)
records what the reference's unmodified utils/derivatives.h returns on them.  A case is a dict: name, objective, x [B, n],
params, config (the mi355_derivative_config fields), hessian (bool), kind and, for planted cases, the expected worst index.

kind   "bits"     compared bit for bit only
       "noise"    Rosenbrock at an ordinary start under the reference's Hessian step: the second difference is rounding
                  noise of the size of f; bit for bit only, no verdict expected across summation orders
       "pass"     both verdicts must be 1, with worst excess < 0.5 in BOTH twin orders (the margin rule)
       "planted"  the verdict named by `fails` must be 0 with worst excess > 2 in both orders and the worst index
                  `worst_index`; the other verdict must be 1 with excess < 0.5

Shapes: the smallest at which the kernels can go wrong: n below, at and above every lane width (8, 16, 32, 64; 128 and 256
coordinates at two and four per lane), B in {1, 5, 13} (no multiple of the 8, 4, 2 segments of a wavefront: padding
segments exist), every stencil, |x_d| on both sides of 1 (both branches of the step)."""
import hashlib
import os

import numpy as np

import dv_lib as T

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "derivatives_reference_vectors.npz")
GRADIENT_N = (1, 2, 8, 9, 16, 17, 33, 64, 65, 129, 256)
HESSIAN_N = (2, 8, 9, 16, 17, 32, 33, 64)
BATCHES = (1, 5, 13)
WIDE_STEP = 2.0 ** -13     # eps^(1/4): the Hessian step that keeps the second difference's rounding noise at eps^(1/2) |f|
DIGEST_ABOVE = 33          # n x n blocks above this n are recorded as SHA-256 digests


def _rng(*key):
    return np.random.default_rng([20261019] + [int(k) for k in key])


def mixed_points(B, n, *key):
    """Coordinates on both sides of |x| = 1: even ones in (-0.9, 0.9), odd ones of size 1.1 .. 3 with either sign."""
    r = _rng(1, B, n, *key)
    x = r.uniform(-0.9, 0.9, size=(B, n))
    big = r.uniform(1.1, 3.0, size=(B, n)) * r.choice([-1.0, 1.0], size=(B, n))
    x[:, 1::2] = big[:, 1::2]
    return x


def near_minimiser(B, n):
    """Rosenbrock's minimiser 1 with every coordinate moved by +-2^-10 (f ~ 1e-3: the reference's step passes there)."""
    r = _rng(2, B, n)
    return 1.0 + r.choice([-1.0, 1.0], size=(B, n)) * 2.0 ** -10


def small_points(B, n, *key):
    return _rng(3, B, n, *key).uniform(-0.5, 0.5, size=(B, n))


def diag_params(n):
    r = _rng(4, n)
    a = r.uniform(0.5, 20.0, size=n) * r.choice([-1.0, 1.0], size=n, p=[0.2, 0.8])
    return np.concatenate([a, [5.0]])


def dense_params(n, symmetric, asymmetry=0.0):
    """S (column major), b, kappa of examples/user_objective_dense.  symmetric: S = (A + A^T) / 2 exactly; `asymmetry`
    is then added to S(0, n - 1) and subtracted from S(n - 1, 0)."""
    r = _rng(5, n)
    A = r.normal(size=(n, n))
    S = (A + A.T) / 2.0 if symmetric else A
    S = S + np.eye(n) * 2.0
    if asymmetry:
        S[0, n - 1] += asymmetry
        S[n - 1, 0] -= asymmetry
    return np.concatenate([np.asfortranarray(S).ravel(order="F"), r.normal(size=n), [0.5]])


def planted_params(n, kind=0, i=0, j=0, size=0.0):
    """Q (column major, exactly symmetric), c, then the plant (kind, i, j, size) of tests/derivatives/planted.hpp."""
    r = _rng(6, n)
    A = r.normal(size=(n, n))
    Q = (A + A.T) / 2.0 + np.eye(n) * 2.0
    return np.concatenate([Q.ravel(order="F"), r.uniform(0.5, 2.0, size=n), [float(kind), float(i), float(j), float(size)]])


def config(accuracy=3, **kw):
    c = dict(gradient_accuracy=accuracy, hessian_accuracy=accuracy, gradient_step=0.0, hessian_step=0.0,
             gradient_tolerance=0.0, hessian_tolerance=0.0)
    c.update(kw)
    return c


def _case(name, objective, x, params=None, hessian=False, kind="bits", **kw):
    c = dict(name=name, objective=objective, x=np.ascontiguousarray(x, dtype=np.float64),
             params=np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64),
             hessian=hessian, kind=kind, config=config())
    c.update(kw)
    return c


def plant_positions(n):
    """0, the last lane of every narrower width, the first lane past it, n - 1."""
    return sorted({p for p in (0, 7, 8, 15, 16, 31, 32, n - 1) if 0 <= p < n})


def make_cases():
    cases = []
    # ---- gradient only: every n, every stencil ------------------------------------------------------------------
    for k, n in enumerate(GRADIENT_N):
        B, acc = BATCHES[k % 3], k % 4
        cases.append(_case("grad_rosenbrock_n%03d_a%d" % (n, acc), T.ROSENBROCK, mixed_points(B, n), config=config(acc)))
        B, acc = BATCHES[(k + 1) % 3], (k + 1) % 4
        cases.append(_case("grad_diag_quadratic_n%03d_a%d" % (n, acc), T.DIAG_QUADRATIC, mixed_points(B, n, 1),
                           diag_params(n), config=config(acc)))
    for n, B, acc in ((1, 5, 3), (9, 13, 0), (65, 1, 2)):
        cases.append(_case("grad_quartic_n%03d_a%d" % (n, acc), T.QUARTIC, mixed_points(B, n, 2), config=config(acc)))
    for n, B, acc in ((2, 13, 1), (17, 5, 3), (65, 1, 0), (129, 5, 2)):   # (65, 129: two and four coordinates per lane)
        cases.append(_case("grad_dense_n%03d_a%d" % (n, acc), T.DENSE, small_points(B, n, 1), dense_params(n, False),
                           config=config(acc)))
    for n, B, acc in ((9, 5, 3), (65, 13, 1), (256, 1, 3)):
        cases.append(_case("grad_planted_n%03d_a%d" % (n, acc), T.PLANTED, small_points(B, n, 2), planted_params(n),
                           config=config(acc)))
    # ---- Hessian: every n, the four-corner and the sixteen-point formula ---------------------------------------------
    for k, n in enumerate(HESSIAN_N):
        for acc in (0, 3):
            B = 13 if (n == 64 and acc == 3) else BATCHES[(k + acc) % 3] if n < 64 else 1
            cases.append(_case("hess_rosenbrock_n%02d_a%d" % (n, acc), T.ROSENBROCK, mixed_points(B, n, 3), hessian=True,
                               kind="noise", config=config(acc)))
    for n, B, acc in ((2, 5, 0), (9, 13, 3), (17, 1, 0), (33, 5, 3), (64, 1, 0)):
        cases.append(_case("hess_diag_quadratic_n%02d_a%d" % (n, acc), T.DIAG_QUADRATIC, mixed_points(B, n, 4),
                           diag_params(n), hessian=True, config=config(acc)))
    for n, B, acc in ((2, 13, 3), (9, 5, 0)):
        cases.append(_case("hess_quartic_n%02d_a%d" % (n, acc), T.QUARTIC, mixed_points(B, n, 5), hessian=True,
                           config=config(acc)))
    for n, B, acc in ((2, 1, 0), (8, 5, 3), (9, 13, 0), (17, 5, 3), (33, 1, 3)):
        cases.append(_case("hess_dense_n%02d_a%d" % (n, acc), T.DENSE, small_points(B, n, 3), dense_params(n, False),
                           hessian=True, config=config(acc)))
    # ---- special points: a coordinate of 0, one of 2^40, one that makes f overflow (NaN passes; nonfinite counted) ----
    x = mixed_points(5, 9, 6)
    x[0, 3] = 0.0
    x[1, 4] = 2.0 ** 40
    x[2, 5] = 1e200
    x[3, 0] = -0.0
    cases.append(_case("special_rosenbrock_n09", T.ROSENBROCK, x, hessian=True, config=config(3)))
    cases.append(_case("special_rosenbrock_n09_a0", T.ROSENBROCK, x, hessian=True, config=config(0)))
    # ---- pass cases ---------------------------------------------------------------------------------------------------
    for n, B in ((2, 13), (9, 5), (33, 1)):
        cases.append(_case("pass_rosenbrock_near_n%02d" % n, T.ROSENBROCK, near_minimiser(B, n), hessian=True, kind="pass"))
    for n, B in ((9, 5), (33, 1)):   # ordinary starts, the wider Hessian step
        cases.append(_case("pass_rosenbrock_wide_step_n%02d" % n, T.ROSENBROCK, mixed_points(B, n, 3), hessian=True,
                           kind="pass", config=config(3, hessian_step=WIDE_STEP)))
    cases.append(_case("pass_dense_symmetric_n17", T.DENSE, small_points(5, 17, 4), dense_params(17, True), hessian=True,
                       kind="pass", config=config(3, hessian_step=WIDE_STEP)))
    # ---- planted cases ------------------------------------------------------------------------------------------------
    for n in (9, 17, 33, 64):
        B = 1 if n == 64 else 5
        x = small_points(B, n, 5)
        pos = plant_positions(n)
        for k in pos:
            if n == 64 and k not in (0, 32, 63):
                continue
            cases.append(_case("planted_gradient_n%02d_k%02d" % (n, k), T.PLANTED, x, planted_params(n, 1, k, 0, 2.0),
                               kind="planted", fails="gradient", worst_index=k))
        pairs = [(pos[0], pos[-1]), (pos[len(pos) // 2 - 1], pos[len(pos) // 2]), (pos[-1], pos[-1])]
        for i, j in pairs:
            # (the symmetric plant: entries (i, j) and (j, i) exceed alike; the first in the column-major array is reported)
            cases.append(_case("planted_hessian_n%02d_i%02d_j%02d" % (n, i, j), T.PLANTED, x,
                               planted_params(n, 2, i, j, 8.0), hessian=True, kind="planted", fails="hessian",
                               worst_index=min(j * n + i, i * n + j), config=config(3, hessian_step=WIDE_STEP)))
        i, j = pairs[1][1], pairs[1][0]   # one side only: H(i, j) alone, i > j
        cases.append(_case("planted_one_sided_n%02d_i%02d_j%02d" % (n, i, j), T.PLANTED, x,
                           planted_params(n, 3, i, j, 8.0), hessian=True, kind="planted", fails="hessian",
                           worst_index=j * n + i, config=config(3, hessian_step=WIDE_STEP)))
    # the dense quartic with H != H^T: the finite Hessian is symmetric, the functor's is not — and g = S x - b is not the
    # gradient of 0.5 x . S x either, so the gradient check fails with it (other_fails): both are real findings
    n = 17
    cases.append(_case("planted_dense_asymmetric_n17", T.DENSE, small_points(5, n, 4), dense_params(n, True, 3.0),
                       hessian=True, kind="planted", fails="hessian", worst_index=None, other_fails=True,
                       worst_among=((n - 1) * n + 0, 0 * n + (n - 1)), config=config(3, hessian_step=WIDE_STEP)))
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def digest(block):
    return hashlib.sha256(np.ascontiguousarray(block, dtype="<f8").tobytes()).hexdigest()


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
