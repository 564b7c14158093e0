"""Plain definitions of the device objectives at 200 bits, and the rounding bounds the device is held to.

TEST INFRASTRUCTURE.  mpmath only: nothing here comes from oracle/, from the package or from the reference tree, and no
formula is written in a kernel's operation order.  Inputs are the exact doubles (or the exact float32 values of the float
kernels) as mpf.

Every objective returns an `Eval`: f, g (and H where the device has hess_full) together with the MAGNITUDE COMPANION
f_abs, g_abs, H_abs — the same formula with every operand replaced by its absolute value and every subtraction by an
addition.  Each formula is therefore written ONCE, over an `_Arith` that says what a subtraction is: `_PLAIN` subtracts,
`_MAGNITUDE` adds (and is handed |operands|).

The bound on a device value v against the definition d with magnitude M is

    |v - d| <= k u M + k eta,      u = 2^-53 (2^-24 float32),  eta = 2^-1074 (2^-149): the kernels do not flush,

k the longest chain of rounded operations an input passes through in the kernel, counted from the arithmetic contract
in the kernel headers and stated beside each formula below (`*_k`).  A pairwise tree counts its depth, a sequential or
fused chain its length.  k is derived, never fitted: tests/test_hp_lib.py shows on the CPU that the twins stay inside
and that wrong kernels (a dropped term, a padding coordinate treated as real, half a gradient) do not.
"""
import math

import mpmath

mp = mpmath.mp.clone()   # a context of its own: the precision of other tests' mpmath work is not touched
mp.prec = 200
mpf = mp.mpf

U = {"float64": mpf(2) ** -53, "float32": mpf(2) ** -24}
ETA = {"float64": mpf(2) ** -1074, "float32": mpf(2) ** -149}


def vec(a):
    """exact mpf of every entry of a numpy vector (float64 or float32)"""
    return [mpf(float(v)) for v in a]


def bound(k, magnitude, dtype="float64"):
    return k * U[dtype] * magnitude + k * ETA[dtype]


def log2_ceil(n):
    return max(0, int(n - 1).bit_length())


class Eval:
    """f, g[j], H[i][j] (None where not asked for) and the magnitude companions f_abs, g_abs, H_abs"""

    def __init__(self, plain, magnitude):
        self.f, self.g, self.H = plain
        self.f_abs, self.g_abs, self.H_abs = magnitude


class _Arith:
    def __init__(self, magnitude):
        self.magnitude = magnitude

    def sub(self, a, b):
        return a + b if self.magnitude else a - b

    def operand(self, v):
        if isinstance(v, (list, tuple)):
            return [self.operand(e) for e in v]
        return abs(v) if self.magnitude else v

    def max0(self, v):
        return v if (self.magnitude or v > 0) else mpf(0)


_PLAIN, _MAGNITUDE = _Arith(False), _Arith(True)


def _both(formula, *operands, **kw):
    return Eval(formula(_PLAIN, *[_PLAIN.operand(o) for o in operands], **kw),
                formula(_MAGNITUDE, *[_MAGNITUDE.operand(o) for o in operands], **kw))


# ---- chained Rosenbrock -------------------------------------------------------------------------------------------------
#   f(x) = sum_{i < n-1} (1 - x_i)^2 + 100 (x_{i+1} - x_i^2)^2                     (n = 1: the empty sum, 0)
#   g_j  = [j < n-1] (-2 (1 - x_j) - 400 x_j (x_{j+1} - x_j^2))  +  [j > 0] 200 (x_j - x_{j-1}^2)
#   H_jj = [j < n-1] (1200 x_j^2 - 400 x_{j+1} + 2) + [j > 0] 200,   H_{j,j+1} = H_{j+1,j} = -400 x_j
def rosenbrock_t1(ar, xi):
    return ar.sub(mpf(1), xi)


def rosenbrock_t2(ar, xi, xnext):
    return ar.sub(xnext, xi * xi)


def rosenbrock_term(ar, xi, xnext):
    t1, t2 = rosenbrock_t1(ar, xi), rosenbrock_t2(ar, xi, xnext)
    return t1 * t1 + 100 * t2 * t2


def rosenbrock_gradient_forward(ar, xi, xnext):
    """d term_i / d x_i"""
    return ar.sub(ar.sub(mpf(0), 2 * rosenbrock_t1(ar, xi)), 400 * xi * rosenbrock_t2(ar, xi, xnext))


def rosenbrock_gradient_backward(ar, xprev, xi):
    """d term_{i-1} / d x_i"""
    return 200 * rosenbrock_t2(ar, xprev, xi)


def _rosenbrock(ar, x, hessian=False):
    n = len(x)
    f = mpf(0)
    for i in range(n - 1):
        f += rosenbrock_term(ar, x[i], x[i + 1])
    g = [mpf(0)] * n
    for j in range(n):
        if j + 1 < n:
            g[j] += rosenbrock_gradient_forward(ar, x[j], x[j + 1])
        if j > 0:
            g[j] += rosenbrock_gradient_backward(ar, x[j - 1], x[j])
    H = None
    if hessian:
        H = [[mpf(0)] * n for _ in range(n)]
        for j in range(n):
            if j + 1 < n:
                H[j][j] += ar.sub(1200 * x[j] * x[j], 400 * x[j + 1]) + 2
                H[j][j + 1] = H[j + 1][j] = ar.sub(mpf(0), 400 * x[j])
            if j > 0:
                H[j][j] += 200
    return f, g, H


def rosenbrock(x, hessian=False):
    return _both(_rosenbrock, vec(x), hessian=hessian)


def rosenbrock_k(n):
    """(k_f, k_g, k_H), objectives.hpp RosenbrockObjectiveT::eval_impl / hess_diag (objectives_f32.hpp: the same order).
    f: x_i -> x_i x_i -> x_{i+1} - . -> 100 . -> . t2 -> t1 t1 + . is a chain of 5 rounded operations, then the pairwise
       tree over the padded width, whose levels above ceil(log2 n) add zeros exactly: ceil(log2 n) + 5 counted, + 1 of
       margin because t2 enters its product twice (the first-order worst case, with t2's two roundings counted in both
       factors, is ceil(log2 n) + 7).  The fused form has fewer roundings per term and a lane chain of at most three
       links in place of two tree levels: no longer.
    g: x x, x' - ., 200 ., . (-2 x), -2 t1 + ., a + b: a chain of 6 for the forward half (the doublings are exact), 4 for
       the backward half, which joins at the last link: 6.
    H: 1200 x, . x, . - 400 x', . + 2, . + 200: 5 on the diagonal (400 x' is one rounding, off the chain), 1 off it."""
    return log2_ceil(n) + 6, 6, 5


# ---- diagonal quadratic --------------------------------------------------------------------------------------------------
#   f(x) = sum_i a_i x_i^2 + c,   g_j = 2 a_j x_j,   H = diag(2 a)
def _diag_quadratic(ar, x, a, c, hessian=False):
    n = len(x)
    f = c
    for i in range(n):
        f += a[i] * x[i] * x[i]
    g = [2 * a[j] * x[j] for j in range(n)]
    H = None
    if hessian:
        H = [[2 * a[j] if i == j else mpf(0) for j in range(n)] for i in range(n)]
    return f, g, H


def diag_quadratic(x, a, c, hessian=False):
    return _both(_diag_quadratic, vec(x), vec(a), mpf(float(c)), hessian=hessian)


def diag_quadratic_k(n):
    """(k_f, k_g, k_H), objectives.hpp DiagQuadraticObjective::eval / eval_fma.
    f: (a x) x is two products, the tree ceil(log2 n) levels, + c one more: ceil(log2 n) + 3 in the exact form.  The fused
       form sums a lane's four coordinates as a chain, a x, (a x) x, then three fused links, where the exact form has two
       products and two tree levels: one longer, ceil(log2 n) + 4, which is the count used for both.
    g: (2 a) x with the doubling exact: 1.  H: 2 a is exact; 1."""
    return log2_ceil(n) + 4, 1, 1


# ---- dense quartic (the example functor, objective 101) ------------------------------------------------------------------
#   f(x) = x . (S x) / 2 - b . x + (kappa / 4) sum_i x_i^4,   g = S x - b + kappa x^3,   H = S + 3 kappa diag(x^2)
# S is used as given (never symmetrised): H_ij = S_ij.
def _dense_quartic(ar, x, S, b, kappa, hessian=False):
    n = len(x)
    sx = [mp.fdot(S[i], x) for i in range(n)]
    f = ar.sub(mp.fdot(x, sx) / 2, mp.fdot(b, x)) + kappa / 4 * sum(v ** 4 for v in x)
    g = [ar.sub(sx[j], b[j]) + kappa * x[j] ** 3 for j in range(n)]
    H = None
    if hessian:
        H = [[S[i][j] + (3 * kappa * x[i] * x[i] if i == j else 0) for j in range(n)] for i in range(n)]
    return f, g, H


def dense_quartic(x, S, b, kappa, hessian=False):
    """S: [n, n] with S[i][j] = S(i, j) (a numpy array or rows of floats)"""
    return _both(_dense_quartic, vec(x), [vec(r) for r in S], vec(b), mpf(float(kappa)), hessian=hessian)


def dense_quartic_k(n):
    """(k_f, k_g, k_H), examples/user_objective_dense/dense_quartic.hpp.
    f: (S x)_i is an ascending chain of n (first term a product), x_i (S x)_i one more, the sum over the coordinates
       ceil(log2 n) levels (a lane's coordinates as an ascending chain: at four per lane three links for two levels, one
       deeper), the halving exact, - b.x and + the quartic part two more: n + ceil(log2 n) + 4.  (b.x and the quartic part,
       x x, q q, the sum, (kappa / 4) . are shorter and join at the last two links.)
    g: the chain of n, - b_i, + kappa (q x): n + 2 (q, q x, kappa . is a chain of 3 that joins at the last link).
    H: 3 kappa, x x, their product, S_ii + .: 4 on the diagonal; off it a copy, exact."""
    return n + log2_ceil(n) + 4, n + 2, 4


# ---- ridge least squares -------------------------------------------------------------------------------------------------
#   f(x) = ||A x - y||^2 + lam ||x||^2,   g = 2 A^T r + 2 lam x,   r = A x - y
# ONE definition for the four device forms (the VALU form, the matrix-core form, the two normal-equation forms).  The
# normal-equation forms compute x^T G x - 2 c^T x + y^T y: its magnitude |x|^T |G| |x| + 2 |c|^T |x| + y^T y is, entry by
# entry, at most the expansion of the magnitude companion below, so the one companion serves them too.
class Ridge:
    def __init__(self, A, lam):
        self.rows, self.n = A.shape
        self.lam = mpf(float(lam))
        self.A = [vec(r) for r in A]
        self.A_abs = [[abs(v) for v in r] for r in self.A]
        self.AT = [list(c) for c in zip(*self.A)]
        self.AT_abs = [list(c) for c in zip(*self.A_abs)]

    def _eval(self, ar, A, AT, x, y):
        r = [ar.sub(mp.fdot(A[i], x), y[i]) for i in range(self.rows)]
        f = mp.fdot(r, r) + self.lam * mp.fdot(x, x)
        g = [2 * mp.fdot(AT[j], r) + 2 * self.lam * x[j] for j in range(self.n)]
        return f, g, None

    def __call__(self, x, y):
        x, y = vec(x), vec(y)
        return Eval(self._eval(_PLAIN, self.A, self.AT, x, y),
                    self._eval(_MAGNITUDE, self.A_abs, self.AT_abs, [abs(v) for v in x], [abs(v) for v in y]))

    def k(self):
        """objectives.hpp SquaredErrorRidgeObjective::eval: r_i is a chain of n multiply-adds and one subtraction, A^T r a
        chain of `rows` more; ridge_mfma_kernel.hpp and ridge_gram.hpp walk the same lengths as fused chains (G and c
        over the rows, G x over n).  n + rows for f and for g."""
        return self.n + self.rows, self.n + self.rows

    def minimiser(self, y):
        """x* of (A^T A + lam I) x = A^T y at 200 bits: Gaussian elimination with partial pivoting (what mp.lu_solve does,
        written over lists — mp.matrix spends more on element access than on the arithmetic), the factors kept for the
        next y.  tests/test_hp_lib.py holds it to mp.lu_solve."""
        n = self.n
        if getattr(self, "_lu", None) is None:
            G = [[None] * n for _ in range(n)]
            for i in range(n):
                for j in range(i, n):
                    G[i][j] = G[j][i] = mp.fdot(self.AT[i], self.AT[j]) + (self.lam if i == j else 0)
            perm = list(range(n))
            for k in range(n):
                p = max(range(k, n), key=lambda i: abs(G[i][k]))
                G[k], G[p], perm[k], perm[p] = G[p], G[k], perm[p], perm[k]
                for i in range(k + 1, n):
                    G[i][k] = m = G[i][k] / G[k][k]          # (the multiplier, kept below the diagonal)
                    row, pivot = G[i], G[k]
                    for j in range(k + 1, n):
                        row[j] -= m * pivot[j]
            self._lu = (G, perm)
        LU, perm = self._lu
        y = vec(y)
        c = [mp.fdot(self.AT[j], y) for j in range(n)]
        z = [c[perm[i]] for i in range(n)]
        for i in range(n):
            z[i] -= mp.fdot(LU[i][:i], z[:i])
        for i in reversed(range(n)):
            z[i] = (z[i] - mp.fdot(LU[i][i + 1:], z[i + 1:])) / LU[i][i]
        return z


# ---- the augmented-Lagrangian composite ----------------------------------------------------------------------------------
#   L(x) = F + sum_i lambda_i c_i + (rho / 2) sum_i c_i^2 + sum_j (1 / (2 rho)) [max(0, mu_j - rho g_j)^2 - mu_j^2]
#   grad = grad F + sum_i (lambda_i + rho c_i) grad c_i - sum_j max(0, mu_j - rho g_j) grad g_j                (rho > 0)
# F, c_i, g_j are TERMS: a primitive, a sum of primitives or the product of two, entering as v, v - k or k - v.
# A term is described as (prims, form, k, product), prims a list of (kind, a, c) with a / c numpy / float or None.
def _primitive(ar, kind, a, c, x):
    n = len(x)
    if kind == "rosenbrock":
        f, g, _ = _rosenbrock(ar, x)
        return f, g
    if kind == "diag_quadratic":
        f, g, _ = _diag_quadratic(ar, x, a, c)
        return f, g
    if kind == "linear":
        return mp.fdot(a, x), list(a)
    if kind == "squared_norm":
        return mp.fdot(x, x), [2 * v for v in x]
    if kind == "squared_affine":
        r = ar.sub(mp.fdot(a, x), c)
        return r * r, [2 * r * a[j] for j in range(n)]
    raise KeyError(kind)


def _term(ar, term, x):
    prims, form, k, product = term
    parts = [_primitive(ar, *p, x) for p in prims]
    n = len(x)
    if product:
        (v1, g1), (v2, g2) = parts
        v, g = v1 * v2, [v2 * g1[j] + v1 * g2[j] for j in range(n)]
    else:
        v, g = sum(p[0] for p in parts), [sum(p[1][j] for p in parts) for j in range(n)]
    if form == "value_minus_k":
        v = ar.sub(v, k)
    elif form == "k_minus_value":
        v, g = ar.sub(k, v), [ar.sub(mpf(0), e) for e in g]
    elif form != "plain":
        raise KeyError(form)
    return v, g


def _composite(ar, x, terms, n_eq, lam, mu, rho):
    n = len(x)
    f, g = _term(ar, terms[0], x)
    g = list(g)
    for i in range(n_eq):
        c, gc = _term(ar, terms[1 + i], x)
        f += lam[i] * c + rho / 2 * c * c
        for j in range(n):
            g[j] += (lam[i] + rho * c) * gc[j]
    for q, t in enumerate(terms[1 + n_eq:]):
        v, gv = _term(ar, t, x)
        active = ar.max0(ar.sub(mu[q], rho * v))
        f += ar.sub(active * active, mu[q] * mu[q]) / (2 * rho)
        for j in range(n):
            g[j] = ar.sub(g[j], active * gv[j])
    return f, g, None


def _mpf_term(ar, t):
    prims, form, k, product = t
    return ([(p[0], None if p[1] is None else ar.operand(vec(p[1])), ar.operand(mpf(float(p[2])))) for p in prims],
            form, ar.operand(mpf(float(k))), product)


def composite(x, terms, n_eq, lam, mu, rho):
    """terms: [objective] + equalities + inequalities, each (prims, form, k, product); lam [n_eq], mu [n_ineq], rho > 0"""
    assert rho > 0
    out = []
    for ar in (_PLAIN, _MAGNITUDE):
        out.append(_composite(ar, ar.operand(vec(x)), [_mpf_term(ar, t) for t in terms], n_eq, ar.operand(vec(lam)),
                              ar.operand(vec(mu)), mpf(float(rho))))
    return Eval(*out)


_PRIMITIVE_K = {"rosenbrock": lambda n: rosenbrock_k(n)[0], "diag_quadratic": lambda n: diag_quadratic_k(n)[0],
                # a x (or x x) and the tree
                "linear": lambda n: log2_ceil(n) + 1, "squared_norm": lambda n: log2_ceil(n) + 1,
                # r = a.x - c is one more, r r doubles what r carries and adds the product
                "squared_affine": lambda n: 2 * (log2_ceil(n) + 2) + 1}


def composite_k(n, terms):
    """auglag_device.hpp AugLagObjective::eval: the sum over the terms of the k of their primitives, plus 4 per constraint —
    multiplier, square, the two scalings of the penalty part and their place in the running sum are at most four roundings
    deep past the term's value.  One k for the value and the gradient (a constraint's value enters the gradient through
    lambda + rho c and through max(0, mu - rho g)).  Loose by construction — a sum where the longest chain would do — and
    still far below any term: tests/test_hp_lib.py drops a term and takes the wrong branch of a max(0, .) to show it."""
    return sum(_PRIMITIVE_K[p[0]](n) for t in terms for p in t[0]) + 4 * (len(terms) - 1)


# ---- norms of what the solvers report ------------------------------------------------------------------------------------
def norm2(v):
    return mp.sqrt(mp.fdot(v, v))


def within(value, definition, k, magnitude, dtype="float64"):
    """(ok, ratio): the device value against the definition.  Where the magnitude is 0 every operand of the formula is 0
    and the value must be exactly 0."""
    v = mpf(float(value))
    if not math.isfinite(float(value)):
        return False, mp.inf
    if magnitude == 0:
        return v == 0, (mpf(0) if v == 0 else mp.inf)
    ratio = abs(v - definition) / bound(k, magnitude, dtype)
    return ratio <= 1, ratio
