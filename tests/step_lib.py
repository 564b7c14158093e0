"""Every iterate of an L-BFGS solve against the textbook definition of the step that produced it, at 200 bits.

TEST INFRASTRUCTURE.  mpmath only (the context of tests/hp_lib.py): nothing here comes from oracle/, from the package or
from the reference tree, and the direction is NOT computed by the two-loop recursion.  Inputs are the exact doubles (or
floats) of a trajectory x_0 .. x_T, g_0 .. g_T, f_0 .. f_T.

The rules of the reference's `Lbfgs::OptimizationStep` (solver/lbfgs.h), restated:
  pairs    s_k = fl(x_{k+1} - x_k), y_k = fl(g_{k+1} - g_k) in the working precision (:248-249): the numbers the kernel
           stores.  Everything after that is at 200 bits.
  store    the pair is stored iff s^T y > eps ||s|| ||y|| (:265-280); the ring has m columns, the oldest is evicted.
  gamma    from the newest pair, stored or not, under three guards (:289-298): y^T y > eps; s^T y / y^T y finite and at
           most 1e7 in absolute value; gamma = max(s^T y / y^T y, eps).  Otherwise the previous gamma stays.
  skip     a stored pair with |s^T y| < eps is left out of the recursion (:165, :189) — of both loops, which is the
           product form without that pair.
  reset    with d = H_k g_k: when -g^T d is not finite or > -eps * eps * max(1, ||x||), the step is steepest descent,
           -g, and the ring is emptied; gamma stays (:214-224).
  H_k      the dense matrix obtained from H_0 by (I - rho s y^T) H (I - rho y s^T) + rho s s^T over the pairs of the
           recursion, oldest to newest, rho = 1 / s^T y; H_0 = gamma I, in Second mode diag(1 / (|H_jj| + eps)) (:133-134).
           For n > DENSE_MAX the same matrix is applied through its compact representation (Byrd, Nocedal, Schnabel 1994,
           eq. 3.1: an identity of the product form, m x m systems only); tests/test_step_lib.py holds the two to 1e-40.
`GradientDescent` (solver/gradient_descent.h:64-73; Rules(solver="gradient_descent")): the same audit with H = I and no
pairs — s a positive multiple of -g_k within the bound with K = 0, the line-search conditions on the solve's own numbers; a
refused search (g.g underflows to 0) steps to x - g.
Dense `Bfgs` (solver/bfgs.h): the same update from H_0 = I over every pair with y^T s > eps ||s|| ||y|| (:125); H back to I
and steepest descent when g^T (-H g) > 0 or NaN (:88-92).

A decision is UNDECIDABLE when its 200-bit margin is inside the rounding slack of the quantities compared; the audit of
that problem stops there and the rest of its iterations count as unaudited.

The bounds.  u = 2^-53 (2^-24), D = the depth of an inner product: ceil(log2 n) + 1 for the kernels' trees, one more where
a lane's coordinates are a fused chain, n for a sequential sum (`Rules.dot`).  With p pairs in the recursion, a coordinate of
the direction passes through
    first loop, per pair:   s.q (D), the division 1 / s^T y and its product (2), alpha y (1), q - . (1)       D + 4
    scaling:                y.y (D), s^T y / y^T y (1), max (0), gamma q (1); Second mode |H| + eps, 1 / ., . q: 3
                            in place of the last                                                          D + 4
    second loop, per pair:  y.r (D), division and product (2), alpha - beta (1), . s (1), r + . (1)          D + 5
    K = p (2 D + 9) + D + 4
rounded operations at the most, each of relative error u against the MAGNITUDE COMPANION M of the recursion (every operand
replaced by its absolute value, every subtraction by an addition).  The inner products s^T y behind rho_i and gamma are
cancelling sums of their own: they enter with the relative error D u |s|^T|y| / s^T y each, carried through the companion
(M' with rho_i, gamma enlarged by it; the part M' - M is added whole, not multiplied by K u).  A fused kernel rounds less
often along the same chain.  The trial point and the stored difference are three more roundings, against the iterates:
    |s_j + alpha d_j| <= alpha (K u / (1 - K u) M'_j + (M'_j - M_j)) + 3 u (|x_k,j| + |x_k+1,j|),    alpha = -(s.d) / (d.d)
(d = H_k g_k, the step runs along -d).  That is the bound b_j on e_j = s_j + t d_j for the step width t the kernel took.  The
audit does not know t: it fits alpha, and alpha - t = -(e.d) / (d.d) moves coordinate j by |alpha - t| |d_j| <=
|d_j| (b.|d|) / (d.d) — a coordinate with a small bound of its own inherits the rounding of the large ones.  That derived term
is the third part of the bound; without it a correct float solve is outside (measured, tests/test_step_lib.py's generator:
2.0 times the two-part bound at Rosenbrock-33, m = 1, where |x_32| is small against the others).
K is counted here and never fitted ("The step as a definition").
"""
import numpy as np

import hp_lib
from hp_lib import mp, mpf

DENSE_MAX = 9            # the dense matrix up to here, the compact representation of the same matrix above
FALLBACK = mpf(10) ** 7  # lbfgs.h:289


def fdot(a, b):
    return mp.fdot(a, b)


def absv(v):
    return [abs(e) for e in v]


class Rules:
    """What was solved: history m, working precision, line search, solver family, and how the code under audit sums an
    inner product ("tree": ceil(log2 n) + 1 deep; "fused": a lane's coordinates as a fused chain, one deeper; "sequential":
    n deep)."""

    def __init__(self, m, dtype="float64", linesearch="more_thuente", solver="lbfgs", second=False, dot="tree",
                 lower=None, upper=None):
        self.m, self.dtype, self.linesearch, self.solver, self.second, self.dot = int(m), dtype, linesearch, solver, second, dot
        self.u = hp_lib.U[dtype]
        self.eps = 2 * self.u            # std::numeric_limits<Scalar>::epsilon()
        self.lower, self.upper = lower, upper
        self.np_dtype = np.float32 if dtype == "float32" else np.float64

    def depth(self, n):
        return n if self.dot == "sequential" else hp_lib.log2_ceil(n) + (2 if self.dot == "fused" else 1)


def direction_K(p, D):
    """the counted K of the module docstring"""
    return p * (2 * D + 9) + D + 4


# ---- H_k g from the definition -------------------------------------------------------------------------------------------
def dense_update(H, s, y, sy):
    """(I - rho s y^T) H (I - rho y s^T) + rho s s^T, rho = 1 / sy"""
    n = len(s)
    rho = 1 / sy
    yH = [fdot(y, [H[i][j] for i in range(n)]) for j in range(n)]                 # y^T H
    A = [[H[i][j] - rho * s[i] * yH[j] for j in range(n)] for i in range(n)]      # (I - rho s y^T) H
    Ay = [fdot(A[i], y) for i in range(n)]
    return [[A[i][j] - rho * Ay[i] * s[j] + rho * s[i] * s[j] for j in range(n)] for i in range(n)]


def dense_H(pairs, h0):
    """pairs: [(s, y, sy)] oldest first; h0: the diagonal of H_0"""
    n = len(h0)
    H = [[h0[i] if i == j else mpf(0) for j in range(n)] for i in range(n)]
    for s, y, sy in pairs:
        H = dense_update(H, s, y, sy)
    return H


def matvec(H, g):
    return [fdot(row, g) for row in H]


def compact_direction(pairs, h0, g):
    """H_k g with H_k = H_0 + [S  H_0 Y] [[R^-T (D + Y^T H_0 Y) R^-1, -R^-T], [-R^-1, 0]] [S^T; Y^T H_0],
    R_ij = s_i^T y_j (i <= j), D = diag(s_i^T y_i)."""
    n, p = len(g), len(pairs)
    h0g = [h0[j] * g[j] for j in range(n)]
    if p == 0:
        return h0g
    S = [q[0] for q in pairs]
    Y = [q[1] for q in pairs]
    h0Y = [[h0[j] * y[j] for j in range(n)] for y in Y]
    R = mp.matrix(p, p)
    W = mp.matrix(p, p)                                   # D + Y^T H_0 Y
    for i in range(p):
        for j in range(p):
            if i <= j:
                R[i, j] = pairs[i][2] if i == j else fdot(S[i], Y[j])
            W[i, j] = fdot(Y[i], h0Y[j]) + (pairs[i][2] if i == j else 0)
    a = mp.matrix([fdot(S[i], g) for i in range(p)])      # S^T g
    b = mp.matrix([fdot(Y[i], h0g) for i in range(p)])    # Y^T H_0 g
    Ria = mp.lu_solve(R, a)
    top = mp.lu_solve(R.T, W * Ria - b)
    out = list(h0g)
    for i in range(p):
        for j in range(n):
            out[j] += S[i][j] * top[i] - h0Y[i][j] * Ria[i]
    return out


def direction(pairs, h0, g, dense=None):
    if dense is None:
        dense = len(g) <= DENSE_MAX
    return matvec(dense_H(pairs, h0), g) if dense else compact_direction(pairs, h0, g)


def magnitude(pairs, h0, g, rho_error=None, h0_error=0):
    """The magnitude companion of the recursion applied to |g|: every operand its absolute value, every subtraction an
    addition; rho_i (1 + rho_error[i]) and H_0 (1 + h0_error) where the relative errors are given."""
    q = absv(g)
    n = len(q)
    alphas = []
    for i in reversed(range(len(pairs))):
        s, y, sy = pairs[i]
        rho = (1 + (rho_error[i] if rho_error else 0)) / sy
        a = rho * fdot(absv(s), q)
        q = [q[j] + a * abs(y[j]) for j in range(n)]
        alphas.append(a)
    alphas.reverse()
    r = [abs(h0[j]) * (1 + h0_error) * q[j] for j in range(n)]
    for i in range(len(pairs)):
        s, y, sy = pairs[i]
        rho = (1 + (rho_error[i] if rho_error else 0)) / sy
        b = rho * fdot(absv(y), r)
        r = [r[j] + abs(s[j]) * (alphas[i] + b) for j in range(n)]
    return r


# ---- the audit -----------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self):
        self.iterations = 0          # traced iterations (steps x_k -> x_k+1)
        self.audited = 0             # with a direction check
        self.unaudited = 0           # after an undecidable decision
        self.exceptions = 0          # line-search tests not met (maxfev, xtol bracket, stpmin / stpmax: not told apart)
        self.audited_through = []    # per problem: (last audited iteration, iterations of the problem)
        self.bad = []
        self.worst = {}              # "direction", "decrease", "curvature", "f", "g": worst error / bound
        self.resets = self.skipped = self.evictions = self.rejected = 0
        self.clipped = 0             # Lbfgsb: steps that reach a bound (no decrease promised)
        self.undecidable = []
        self.exception_notes = []

    def see(self, key, ratio):
        self.worst[key] = max(self.worst.get(key, 0.0), float(ratio))

    def merge(self, other):
        for k in ("iterations", "audited", "unaudited", "exceptions", "resets", "skipped", "evictions", "rejected", "clipped"):
            setattr(self, k, getattr(self, k) + getattr(other, k))
        self.audited_through += other.audited_through
        self.bad += other.bad
        self.undecidable += other.undecidable
        self.exception_notes += other.exception_notes
        for k, v in other.worst.items():
            self.see(k, v)

    def line(self):
        return ("%d iterations, %d unaudited, %d exceptions, %d resets, %d evictions, %d pairs rejected%s, worst %s"
                % (self.iterations, self.unaudited, self.exceptions, self.resets, self.evictions, self.rejected,
                   ", %d steps reach a bound" % self.clipped if self.clipped else "",
                   ", ".join("%s %.3g" % kv for kv in sorted(self.worst.items()))))


MAX_OUTSIDE = mpf(2) / 100    # of the traced iterations of a case: unaudited or line-search exceptions


def caps(report, m):
    """The two conditions on a case (conditions, not measurements): at most 2 % of the traced iterations unaudited or
    line-search exceptions, and every problem audited through iteration 2 m + 2 (or its end, where it ends sooner)."""
    out = []
    if report.iterations == 0:
        out.append("no traced iteration")
    elif mpf(report.unaudited + report.exceptions) / report.iterations > MAX_OUTSIDE:
        out.append("%d unaudited + %d exceptions of %d iterations: more than 2 %%"
                   % (report.unaudited, report.exceptions, report.iterations))
    for i, (through, total) in enumerate(report.audited_through):
        if through < min(total, 2 * m + 2):
            out.append("problem %d audited through iteration %d of %d, needs %d" % (i, through, total, min(total, 2 * m + 2)))
    return out


def _slack_of_dot(g, s, xa, xb, D, u):
    """rounding of the kernel's own g^T d and alpha, in terms of s = fl(x_k+1 - x_k): the inner product over the direction
    (D), the step's product and the slope's (2), and the three roundings between alpha d_j and s_j"""
    n = len(g)
    return (D + 2) * u * fdot(absv(g), absv(s)) + 3 * u * sum(abs(g[j]) * (abs(xa[j]) + abs(xb[j])) for j in range(n))


def _line_search(rules, rep, what, f0, f1, g0, g1, s, xa, xb, D):
    u = rules.u
    phi0, phi1 = fdot(g0, s), fdot(g1, s)
    sl0, sl1 = _slack_of_dot(g0, s, xa, xb, D, u), _slack_of_dot(g1, s, xa, xb, D, u)
    fround = 3 * u * (abs(f0) + abs(phi0))
    if rules.linesearch == "more_thuente" or rules.solver == "lbfgsb":
        c1 = mpf(1) / 10000
        decrease = f1 <= f0 + c1 * phi0 + c1 * sl0 + fround
        rep.see("decrease", (f1 - f0 - c1 * phi0) / (c1 * sl0 + fround) if f1 > f0 + c1 * phi0 else 0)
        if rules.solver == "lbfgsb":           # a step may be clipped at the box: the first inequality only
            ok = decrease
        else:
            c2 = mpf(9) / 10
            slack = sl1 + c2 * sl0 + 2 * u * abs(phi0)
            ok = decrease and abs(phi1) <= c2 * abs(phi0) + slack
    else:                                      # hager_zhang.h:133-138, delta = 0.1, sigma = 0.9, epsilon = 1e-6
        delta, sigma, epsilon = mpf(1) / 10, mpf(9) / 10, mpf(10) ** -6
        slack = sl1 + sl0 + 2 * u * abs(phi0)
        curvature = phi1 >= sigma * phi0 - slack
        t1 = delta * phi0 + delta * sl0 + fround >= f1 - f0 and curvature
        t2 = (2 * delta - 1) * phi0 + slack >= phi1 and curvature and f1 <= f0 + epsilon * abs(f0) + fround
        ok = t1 or t2
    if not ok:
        rep.exceptions += 1
        rep.exception_notes.append("%s: f %s -> %s, g^T s %s -> %s" % (what, mp.nstr(f0, 17), mp.nstr(f1, 17), mp.nstr(phi0, 6),
                                                                     mp.nstr(phi1, 6)))
    return ok


def audit_problem(xs, gs, fs, rules, hess_diag=None, what=""):
    """xs, gs [T + 1, n], fs [T + 1]: x_0 .. x_T of one problem in the working precision.  hess_diag(x) -> the 200-bit
    diagonal of the Hessian at x (Second mode).  Returns a Report."""
    rep = Report()
    T, n = len(xs) - 1, len(xs[0])
    u, eps = rules.u, rules.eps
    D = rules.depth(n)
    X = [hp_lib.vec(x) for x in xs]
    G = [hp_lib.vec(g) for g in gs]
    F = [mpf(float(f)) for f in fs]
    work = rules.np_dtype
    ring, gamma, gamma_error = [], mpf(1), mpf(0)      # ring: [(s, y, sy, |s|^T|y|)] oldest first
    H = Habs = None                                    # dense Bfgs
    updates = 0
    alive = True
    rep.iterations = T
    through = 0

    def undecidable(why, k):
        rep.undecidable.append("%s iteration %d: %s" % (what, k + 1, why))

    for k in range(T):
        s = hp_lib.vec(np.asarray(xs[k + 1], dtype=work) - np.asarray(xs[k], dtype=work))
        y = hp_lib.vec(np.asarray(gs[k + 1], dtype=work) - np.asarray(gs[k], dtype=work))
        g = G[k]
        if rules.solver == "lbfgsb":
            lo, hi = rules.lower, rules.upper
            if not all(lo[j] <= xs[k + 1][j] <= hi[j] for j in range(n)):
                rep.bad.append("%s iteration %d: an iterate outside its box" % (what, k + 1))
            # lbfgsb.h:187-203: with no free variable the step is the Cauchy point without a search, and a point past the box
            # is projected back and evaluated again: a coordinate that REACHES a bound in this step may have been put there by
            # either, s is then no multiple of the direction searched and no decrease is promised.  Every other step is
            # x + t d with the search's t: the first inequality holds along s.
            reaches = any((xs[k + 1][j] == lo[j] and xs[k][j] != lo[j]) or (xs[k + 1][j] == hi[j] and xs[k][j] != hi[j])
                          for j in range(n))
            if reaches:
                rep.clipped += 1
            else:
                _line_search(rules, rep, "%s iteration %d" % (what, k + 1), F[k], F[k + 1], g, G[k + 1], s, X[k], X[k + 1], D)
            rep.audited += 1
            through = k + 1
            continue
        if alive:
            reset = False
            steepest = rules.solver == "gradient_descent"      # H = I and no pairs: the direction is g itself
            if steepest:
                # gradient_descent.h:64-73 searches along -g from x_k.  The refused search is a rule: where g.g underflows to
                # 0 the search returns its initial step 1 and the iterate is x - g, evaluated again (more_thuente.h:152-156)
                if all(float(e) * float(e) == 0.0 for e in g):
                    if not np.array_equal(np.asarray(xs[k + 1], dtype=work),
                                          np.asarray(xs[k], dtype=work) - np.asarray(gs[k], dtype=work)):
                        rep.bad.append("%s iteration %d: a refused search did not step to x - g" % (what, k + 1))
                    rep.audited += 1
                    through = k + 1
                    continue
            elif rules.solver == "bfgs":
                if H is None:
                    H = [[mpf(1) if i == j else mpf(0) for j in range(n)] for i in range(n)]
                    Habs = [row[:] for row in H]
                    updates = 0
                d = matvec(H, g)
                M1 = M0 = matvec(Habs, absv(g))
                # per update: H y (n), y^T H y (n), rho, and five operations per entry; then the product H g (n)
                K = updates * (2 * n + 8) + n
                gd = fdot(g, d)
                slack = K * u * fdot(absv(g), M1) + D * u * fdot(absv(g), absv(d))
                if abs(gd) <= slack:
                    undecidable("g^T H g = %s within %s of 0" % (mp.nstr(gd, 5), mp.nstr(slack, 5)), k)
                    alive = False
                elif gd < 0:                  # bfgs.h:88: phi = g^T (-H g) > 0
                    reset = True
                    H = None
            else:
                live, rho_error = [], []
                for (ps, py, sy, say) in ring:
                    if abs(abs(sy) - eps) <= D * u * say:
                        undecidable("|s^T y| = %s against eps" % mp.nstr(sy, 5), k)
                        alive = False
                        break
                    if abs(sy) < eps:         # lbfgs.h:165, :189
                        rep.skipped += 1
                        continue
                    live.append((ps, py, sy))
                    rho_error.append(D * u * say / abs(sy))
            if alive and rules.solver == "lbfgs":
                if rules.second:
                    h0 = [1 / (abs(h) + eps) for h in hess_diag(xs[k])]       # lbfgs.h:133-134
                    h0_error = mpf(0)
                else:
                    h0, h0_error = [gamma] * n, gamma_error
                d = direction(live, h0, g)
                M0 = magnitude(live, h0, g)
                M1 = magnitude(live, h0, g, rho_error, h0_error)
                K = direction_K(len(live), D)
                # lbfgs.h:214-215: descent = -g^T d > -eps * eps * max(1, ||x||)
                gd = fdot(g, d)
                threshold = eps * eps * max(mpf(1), hp_lib.norm2(X[k]))
                gM = fdot(absv(g), M1)
                slack = (K + D) * u * gM + fdot(absv(g), [M1[j] - M0[j] for j in range(n)]) + (D + 3) * u * threshold
                if abs(gd - threshold) <= slack:
                    undecidable("g^T d = %s against the reset threshold %s, slack %s"
                                % (mp.nstr(gd, 5), mp.nstr(threshold, 5), mp.nstr(slack, 5)), k)
                    alive = False
                elif gd < threshold:
                    reset = True
                    ring = []                 # lbfgs.h:219-220; gamma stays
            if alive:
                if reset:
                    rep.resets += 1
                if reset or steepest:
                    d, M0, M1, K = g, absv(g), absv(g), 0
                dd = fdot(d, d)
                alpha = -fdot(s, d) / dd if dd > 0 else mpf(0)
                if not alpha > 0:
                    rep.bad.append("%s iteration %d: the step is no positive multiple of -H g (alpha = %s)"
                                   % (what, k + 1, mp.nstr(alpha, 5)))
                else:
                    Ku = K * u / (1 - K * u)
                    own = [alpha * (Ku * M1[j] + (M1[j] - M0[j])) + 3 * u * (abs(X[k][j]) + abs(X[k + 1][j]))
                           + 3 * hp_lib.ETA[rules.dtype] for j in range(n)]
                    fit = fdot(own, absv(d)) / dd          # |alpha - step|: what the fitted alpha takes from the others
                    for j in range(n):
                        bound = own[j] + fit * abs(d[j])
                        err = abs(s[j] + alpha * d[j])
                        rep.see("direction", err / bound)
                        if err > bound:
                            rep.bad.append("%s iteration %d coordinate %d: |s + alpha d| = %s, bound %s (K = %d, %d pairs)"
                                           % (what, k + 1, j, mp.nstr(err, 5), mp.nstr(bound, 5), K,
                                              len(live) if rules.solver == "lbfgs" and not reset else 0))
                            break
                rep.audited += 1
                through = k + 1
        if not alive:
            rep.unaudited += 1
        _line_search(rules, rep, "%s iteration %d" % (what, k + 1), F[k], F[k + 1], g, G[k + 1], s, X[k], X[k + 1], D)
        if not alive or rules.solver == "gradient_descent":      # (gradient descent keeps no state)
            continue
        # ---- the state after the step -------------------------------------------------------------------------------------
        sy, say = fdot(s, y), fdot(absv(s), absv(y))
        ss, yy = fdot(s, s), fdot(y, y)
        rhs = eps * mp.sqrt(ss) * mp.sqrt(yy)
        if abs(sy - rhs) <= D * u * say + (D + 4) * u * rhs and not (sy == 0 and rhs == 0):
            if k + 1 < T:
                undecidable("s^T y = %s against eps ||s|| ||y|| = %s" % (mp.nstr(sy, 5), mp.nstr(rhs, 5)), k)
            alive = False
            continue
        store = sy > rhs                       # lbfgs.h:267, bfgs.h:125
        if not store:
            rep.rejected += 1
        if rules.solver == "bfgs":
            if store:
                if H is None:
                    H = [[mpf(1) if i == j else mpf(0) for j in range(n)] for i in range(n)]
                    Habs = [row[:] for row in H]
                    updates = 0
                H = dense_update(H, s, y, sy)
                # the companion of the update: rho against |s|^T|y| carries its own error whole
                rho_abs = (1 + D * u * say / sy) / sy
                sa, ya = absv(s), absv(y)
                yH = [fdot(ya, [Habs[i][j] for i in range(n)]) for j in range(n)]
                A = [[Habs[i][j] + rho_abs * sa[i] * yH[j] for j in range(n)] for i in range(n)]
                Ay = [fdot(A[i], ya) for i in range(n)]
                Habs = [[A[i][j] + rho_abs * Ay[i] * sa[j] + rho_abs * sa[i] * sa[j] for j in range(n)] for i in range(n)]
                updates += 1
            continue
        if store:
            if len(ring) == rules.m:
                ring.pop(0)                    # lbfgs.h:275-278: the oldest
                rep.evictions += 1
            ring.append((s, y, sy, say))
        # lbfgs.h:289-298
        if abs(yy - eps) <= D * u * yy:
            if k + 1 < T:
                undecidable("y^T y = %s against eps" % mp.nstr(yy, 5), k)
            alive = False
            continue
        if yy > eps:
            temp = sy / yy
            temp_error = D * u * say / abs(sy) if sy != 0 else mpf(0)
            if abs(abs(temp) - FALLBACK) <= (temp_error + (D + 1) * u) * abs(temp) or \
                    abs(temp - eps) <= (temp_error + (D + 1) * u) * abs(temp):
                if k + 1 < T:
                    undecidable("gamma = %s against its guards" % mp.nstr(temp, 5), k)
                alive = False
                continue
            if abs(temp) <= FALLBACK:
                gamma, gamma_error = (temp, temp_error) if temp > eps else (eps, mpf(0))
    rep.audited_through.append((through, T))
    return rep


def audit_values(evaluate, ks, xs, gs, fs, dtype, rep, what="", first=0):
    """the traced value and gradient of every iterate against the definition, within the bounds of tests/hp_lib.py"""
    import hp_cases

    class _W:
        def see(self, label, ratio):
            rep.see(label, ratio)

    for k in range(first, len(xs)):
        rep.bad += hp_cases.audit(evaluate(xs[k]), fs[k], gs[k], ks, dtype, worst=_W(), what="%s iterate %d" % (what, k))


def audit_case(trajectories, rules, evaluate=None, ks=None, hess_diag=None, what="", first_value=0):
    """trajectories: [(xs, gs, fs)] of the traced problems of one case -> the merged Report"""
    total = Report()
    for i, (xs, gs, fs) in enumerate(trajectories):
        rep = audit_problem(xs, gs, fs, rules, hess_diag=hess_diag, what="%s problem %d" % (what, i))
        if evaluate is not None:
            audit_values(evaluate, ks, xs, gs, fs, rules.dtype, rep, what="%s problem %d" % (what, i), first=first_value)
        total.merge(rep)
    return total


# ---- a plain trajectory generator that can carry planted bugs -----------------------------------------------------------------
# Lbfgs::OptimizationStep as the reference writes it (two loops over a ring of m columns), in numpy in the working
# precision with a pairwise tree for every inner product, under a bracketing search for the strong Wolfe conditions
# (1e-4, 0.9).  Without a bug its trajectories pass the audit; tests/test_step_lib.py plants each bug and shows that the
# audit sees it.
EVICT_NEWEST = "the newest pair is evicted instead of the oldest, once the ring is full"
RING_ONE_OFF = "the ring is read one column off after the first wrap"
GAMMA_OLDEST = "gamma is taken from the oldest stored pair"
SECOND_LOOP_REVERSED = "the second loop pairs alpha_i with the wrong column (its index reversed)"
SECOND_AS_GAMMA = "Second mode with gamma I in place of the diagonal"
DECREASE_ALONE = "the search accepts on sufficient decrease alone"
BUGS = (EVICT_NEWEST, RING_ONE_OFF, GAMMA_OLDEST, SECOND_LOOP_REVERSED, SECOND_AS_GAMMA, DECREASE_ALONE)


def tree_dot(a, b):
    p = a * b
    width = 1 << hp_lib.log2_ceil(max(1, p.size))
    p = np.concatenate([p, np.zeros(width - p.size, dtype=p.dtype)])
    while p.size > 1:
        p = p[0::2] + p[1::2]
    return p[0]


def generate(fun, x0, m, limit, gradient_norm=1e-6, dtype=np.float64, bug=None, hess_diag=None):
    """fun(x) -> (f, g) in `dtype`; hess_diag(x) -> diag H(x) in `dtype` (Second mode).  Returns xs, gs [T + 1, n],
    fs [T + 1] with T <= limit + 1 iterations, ended by |g|_inf < gradient_norm max(1, |x|_inf)."""
    t = dtype
    eps = t(np.finfo(t).eps)
    x = np.asarray(x0, dtype=t)
    n = x.size
    f, g = fun(x)
    S, Y = np.zeros((n, m), dtype=t), np.zeros((n, m), dtype=t)
    count = pos = 0
    wrapped = False
    gamma = t(1)
    xs, gs, fs = [x], [g], [f]
    for _ in range(limit + 1):
        d = g.copy()
        k = count
        off = 1 if (bug == RING_ONE_OFF and wrapped) else 0
        column = lambda i: i if count < m else (pos + i + off) % m
        alpha = np.zeros(m, dtype=t)
        for i in reversed(range(k)):
            c = column(i)
            denom = tree_dot(S[:, c], Y[:, c])
            if abs(denom) < eps:
                continue
            alpha[i] = (t(1) / denom) * tree_dot(S[:, c], d)
            d = d - alpha[i] * Y[:, c]
        if hess_diag is not None and bug != SECOND_AS_GAMMA:
            d = (t(1) / (np.abs(hess_diag(x)) + eps)) * d
        else:
            d = d * gamma
        for i in range(k):
            c = column(i)
            denom = tree_dot(S[:, c], Y[:, c])
            if abs(denom) < eps:
                continue
            beta = (t(1) / denom) * tree_dot(Y[:, c], d)
            d = d + S[:, c] * (alpha[k - 1 - i if bug == SECOND_LOOP_REVERSED else i] - beta)
        descent = -tree_dot(g, d)
        step = t(1)
        if count == 0:
            norm = np.sqrt(tree_dot(d, d))
            step = t(1) / norm if norm > eps else t(1)
        if not np.isfinite(descent) or descent > -eps * eps * max(t(1), np.sqrt(tree_dot(x, x))):
            d = g.copy()
            count = pos = 0
            wrapped = False
            norm = np.sqrt(tree_dot(g, g))
            step = t(1) / norm if norm > eps else t(1)
        direction = -d
        slope0 = tree_dot(g, direction)
        low, high = t(0), None
        for _trial in range(60):
            xn = x + step * direction
            fn, gn = fun(xn)
            slope = tree_dot(gn, direction)
            if not fn <= f + t(1e-4) * step * slope0:
                high = step
            elif bug == DECREASE_ALONE or abs(slope) <= t(0.9) * (-slope0):
                break
            elif slope < 0:
                low = step
            else:
                high = step
            step = (low + high) / t(2) if high is not None else step * t(4)
        s, y = xn - x, gn - g
        sy = tree_dot(s, y)
        if sy > eps * np.sqrt(tree_dot(s, s)) * np.sqrt(tree_dot(y, y)):
            if count < m:
                S[:, count], Y[:, count] = s, y
                count += 1
            elif bug == EVICT_NEWEST:
                c = (pos + m - 1) % m
                S[:, c], Y[:, c] = s, y
            else:
                S[:, pos], Y[:, pos] = s, y
                pos = (pos + 1) % m
                wrapped = True
        yy = tree_dot(y, y)
        if bug == GAMMA_OLDEST and count > 0:
            c = 0 if count < m else pos
            scaling = tree_dot(Y[:, c], S[:, c]) / tree_dot(Y[:, c], Y[:, c])
            gamma = max(scaling, eps)
        elif yy > eps:
            scaling = tree_dot(y, s) / yy
            if np.isfinite(scaling) and abs(scaling) <= t(1e7):
                gamma = max(scaling, eps)
        x, f, g = xn, fn, gn
        xs.append(x)
        gs.append(g)
        fs.append(f)
        if np.max(np.abs(g)) < t(gradient_norm) * max(t(1), np.max(np.abs(x))):
            break
    return np.array(xs), np.array(gs), np.array(fs)
