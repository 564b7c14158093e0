"""Every iterate of a TrustRegionNewton, NewtonDescent, ConjugatedGradientDescent or GradientDescent solve against the textbook
definition of the step that produced it, at 200 bits.

TEST INFRASTRUCTURE.  mpmath only (the context of tests/hp_lib.py), with the Rules, the Report base and the two caps of
tests/step_lib.py and the componentwise solve of tests/bstep_lib.py: nothing here comes from oracle/, from the package, from
the twins or from the reference tree.  Inputs are the exact doubles of a trajectory x_0 .. x_T, g_0 .. g_T, f_0 .. f_T and the
per-iteration counts d nfev, d sum_k of the progress record.  H(x_k) is the definition's (tests/hp_lib.py), never a traced one.

These steps have almost no hidden state: each is a function of (x_k, g_k, H(x_k)) and one scalar (the radius) or one vector
(d_{k-1}), both replayed from the trajectory.  The rules, restated from the reference's headers:

TrustRegionNewton (solver/trust_region_newton.h:190-298, :339-451)
  radius   a working-precision scalar, replayed in double: r * shrink_factor when rho < rho_low; min(expand_factor * r,
           max_radius) when rho > rho_high AND the subproblem ended on the boundary; else unchanged.
  CG       Steihaug's iteration on (H, g_k, r) at 200 bits.  Tolerance coef * min(0.5, sqrt |g|_inf) * |g|_inf; the early exit
           (|g|_2 <= tolerance: the zero step); at most `cg_max_iterations_floor` iterations (InitializeSolver sets dim_ and
           ResetInternal zeroes it again: the cap is the floor alone — a rule); curvature <= 0 and |p + alpha d| >= r end on
           the boundary with the positive root tau = (-b + sqrt(b^2 - 4 a c)) / (2 a).
  rho      (f_k - f(x_k + p)) / (-g.p - p^T H p / 2), -inf where the predicted reduction is <= 0; accepted when rho >
           acceptance_threshold; else retried at the new radius, up to rejection_retry_limit times, ended by radius <=
           min_radius.  A rejected retry's f(x_k + p) is the definition's at 200 bits; the accepted one's is the device's own
           f_k+1, on which rho must exceed the threshold.
  counts   d sum_k = the CG iterations of every retry; d nfev = 1 + 1 per retry + 1 on acceptance.  A retry that leaves the
           radius where it was would repeat itself to the limit: the remaining retries are counted, not run (the kernel's
           documented shortcut; the same numbers as running them).
  a stalled step (x_k+1 = x_k) must be what the rules give: retries exhausted, the radius at min_radius, or the radius stuck.
  Decision-independent on every accepted step: |s|_2 <= r + slack; predicted reduction of s > 0; model(s) <= model(Cauchy
  point within r) + slack (Steihaug's guarantee).
NewtonDescent (solver/newton_descent.h:66-81, linesearch/armijo.h:82-102)
  d* = -(H + safe_guard I)^-1 g_k by a 200-bit solve.  alpha is KNOWN: t = d sum_k - 1 rejected trials, alpha the double of t
  successive fl(alpha * rho) from 1.  cache = c g.d + ((c / 2) c) d^T H d; the accepted trial has f_k+1 <= f_k + alpha cache,
  and with t > 0 the trial before it (value from the definition at x_k + alpha_prev d*) fails that.  The kernel's one
  departure, the bounded search, is a rule: a search that ended on alpha * rho == alpha promises no decrease.
ConjugatedGradientDescent (solver/conjugated_gradient_descent.h:62-85, linesearch/armijo.h:45-64)
  d_0 = -g_0, d_k = -g_k + (g_k.g_k / g_k-1.g_k-1) d_k-1 from the traced gradients alone; alpha known as above; cache = c g.d;
  the same two Armijo checks.  A search that ran to alpha <= alpha_min (176 trials at the defaults) promises no decrease:
  the reference's behaviour where Fletcher-Reeves stops being a descent direction.
GradientDescent (solver/gradient_descent.h:64-73): tests/step_lib.py with Rules(solver="gradient_descent") — its direction
  and line-search audit with H = I and no pairs; and where the search took one trial (d sum_k = 1) it accepted its initial
  step 1: s = -g_k within 3 u (|x_k| + |x_k+1|), nothing fitted.

The bounds ("The Newton and first-order steps as definitions").  u = 2^-53; D = ceil(log2 W) + 1, the
segment butterfly over the padded width W = max(8, 2^ceil(log2 n)) with its product (the levels above that add zeros
exactly), D = n in the reference's sequential order; k_H the count of an entry of the device's H against its magnitude
companion |H|.  Each is a first-order bound against magnitude companions, counted, never fitted:
  Newton descent   d: Skeel's componentwise form |A^-1| (3 n u |L||U| + e_A) |d*|, |L||U| from the partially pivoted
                   factorisation at 200 bits, e_A = k_H u |H| + u (|H_ii| + safe_guard) on the diagonal.
                   |s_j - alpha d*_j| <= alpha e_d,j + 3 u (|x_k,j| + |x_k+1,j|).
                   cache: c ((D + 2) u |g|.|d| + |g|.e_d) + kq ((n + D + 2 + k_H) u |d|^T|H||d| + 2 (|H||d|).e_d) + u |cache|
                   ((kq d)^T H is an ascending chain of n, then a butterfly); a trial: alpha e_cache + 2 u (|f_k| + alpha
                   |cache|), and for the trial before, whose value is the definition's, k_f u f_abs + |g(trial)|.(alpha e_d +
                   2 u |trial|) more.
  Fletcher-Reeves  a RUNNING bound e_k through the recurrence: beta carries (2 D + 1) u (two sums of squares, a division),
                   e_k = beta e_k-1 + (2 D + 2) u beta |d_k-1| + u |d_k|;  |s_j - alpha d_k,j| <= alpha e_k,j + 3 u (|x_k,j| +
                   |x_k+1,j|);  cache: c ((D + 2) u |g|.|d| + |g|.e_k) + u |cache|.
  trust region     a RUNNING bound through Steihaug's recurrence (e_p, e_r, e_d and the scalars): H d is an ascending chain
                   of n, (n + k_H) u |H||d| + |H| e_d; every inner product D u against the product of absolute values plus
                   its operands' errors; alpha, beta by the quotient rule; every vector update two roundings.  The boundary
                   root carries a, b, c, the discriminant (which cancels: its error is absolute) and the numerator -b + sqrt
                   the same way.  |s_j - p_j| <= e_p,j + 3 u (|x_k,j| + |x_k+1,j|).  The predicted reduction: D u |g|.|p| +
                   |g|.e_p + ((n + k_H + D) u |p|^T|H||p| + 2 (|H||p|).e_p) / 2 + 2 u (|g.p| + |p^T H p| / 2); rho by the quotient
                   rule, with k_f u f_abs + |g(trial)|.(e_p + 2 u |trial|) for a rejected trial's value.
A decision whose 200-bit margin lies inside the slack of what it compares is UNDECIDABLE: the CG stopping tests, the curvature
sign, the boundary crossing, the sign of the predicted reduction, rho against its three thresholds.  The audit of that problem
ends there (the radius is no longer known).  NewtonDescent and ConjugatedGradientDescent have no such decision: alpha is
known, and an Armijo trial inside its slack is consistent with either outcome.

The magnitudes |A^-1| and |L||U| multiply u: they are evaluated in double FROM the 200-bit factors and enlarged by 1e-6 (the
double inverse is checked against A; a matrix it does not invert to 1e-7 goes through mp.inverse).  The values — d*, p, tau,
rho, every margin — are at 200 bits.
"""
import numpy as np

import bstep_lib
import hp_cases
import hp_lib
import step_lib
from hp_lib import mp, mpf
from step_lib import absv, fdot

INF = mpf("inf")
# the caps of step_lib.caps (every problem audited through iteration 2 m + 2): 10 for the Newton solvers, 20 for the others
CAP_M = {"trust_region": 4, "newton_descent": 4, "conjugated_gradient": 9, "gradient_descent": 9}
DEFAULTS = {
    "trust_region": dict(initial_radius=1.0, max_radius=1e10, acceptance_threshold=0.15, shrink_factor=0.25,
                         expand_factor=2.0, rho_low=0.25, rho_high=0.75, cg_forcing_coefficient=0.5,
                         cg_max_iterations_floor=10, min_radius=1e-12, rejection_retry_limit=50),   # trust_region_newton.h
    "newton_descent": dict(safe_guard=1e-5, armijo_c=0.2, armijo_rho=0.9),                        # newton_descent.h:69
    "conjugated_gradient": dict(armijo_c=0.2, armijo_rho=0.9, armijo_alpha_min=1e-8),             # armijo.h:49-56
    "gradient_descent": {},
}


class Rules(step_lib.Rules):
    """solver, its config (the reference's defaults where not given) and the order of an inner product"""

    def __init__(self, solver, dot="tree", config=None):
        super().__init__(CAP_M[solver], solver=solver, dot=dot)
        self.config = dict(DEFAULTS[solver], **(config or {}))

    def depth(self, n):
        return n if self.dot == "sequential" else hp_lib.log2_ceil(max(n, 8)) + 1

    def key(self):
        return (self.solver, self.dot, tuple(sorted(self.config.items())))


BRANCHES = ("cg_zero", "cg_tolerance", "cg_negative", "cg_boundary", "cg_cap", "retries", "shrinks", "grows", "stalls",
            "armijo_first", "armijo_later", "no_promise")


class Report(step_lib.Report):
    """step_lib.Report and the branches a case went through: how each CG-Steihaug run ended, rejected retries, radius
    shrinks and growths, stalled steps; Armijo searches that accepted their first trial and a later one; searches that
    promise no decrease (alpha_min, the fixed point of alpha * rho)"""

    def __init__(self):
        super().__init__()
        for b in BRANCHES:
            setattr(self, b, 0)

    def merge(self, other):
        super().merge(other)
        for b in BRANCHES:
            setattr(self, b, getattr(self, b) + getattr(other, b, 0))

    def branches(self):
        return {b: getattr(self, b) for b in BRANCHES}

    def line(self):
        return ("%d iterations, %d unaudited, %d exceptions, %s, worst %s"
                % (self.iterations, self.unaudited, self.exceptions,
                   " ".join("%s %d" % (b, getattr(self, b)) for b in BRANCHES if getattr(self, b)),
                   ", ".join("%s %.3g" % kv for kv in sorted(self.worst.items()))))


class Undecidable(Exception):
    pass


def _decide(margin, slack, why):
    if abs(margin) <= slack:
        raise Undecidable("%s: margin %s inside slack %s" % (why, mp.nstr(margin, 5), mp.nstr(slack, 5)))


def _lu(A):
    """bstep_lib._lu — partial pivoting at 200 bits -> (perm, L, U), A[perm[i]] = (L U)[i] — over the trailing block only and
    past the zeros of a banded matrix (Rosenbrock's H is tridiagonal, the quadratic's diagonal)"""
    k = len(A)
    A = [row[:] for row in A]
    perm = list(range(k))
    for c in range(k):
        piv = max(range(c, k), key=lambda r: abs(A[r][c]))
        A[c], A[piv], perm[c], perm[piv] = A[piv], A[c], perm[piv], perm[c]
        pivot = A[c]
        live = [j for j in range(c + 1, k) if pivot[j] != 0]
        for r in range(c + 1, k):
            row = A[r]
            if row[c] != 0:
                row[c] = m = row[c] / pivot[c]
                for j in live:
                    row[j] -= m * pivot[j]
    L = [[A[i][j] if j < i else mpf(1 if i == j else 0) for j in range(k)] for i in range(k)]
    U = [[A[i][j] if j >= i else mpf(0) for j in range(k)] for i in range(k)]
    return perm, L, U


class Solve(bstep_lib.Solve):
    """bstep_lib.Solve with the values from a 200-bit partially pivoted factorisation over lists and the two magnitudes
    |A^-1|, |L||U| in double from those factors (see the head of this module)"""

    def __init__(self, A, eA=None):
        k = self.k = len(A)
        self.A = A
        perm, L, U = _lu(A)
        self.perm, self.L, self.U = perm, L, U
        Lf = np.array([[float(v) for v in r] for r in L])
        Uf = np.array([[float(v) for v in r] for r in U])
        Af = np.array([[float(v) for v in r] for r in A])
        LU = (np.abs(Lf) @ np.abs(Uf)) * (1 + 1e-6)
        inv = np.linalg.inv(Af)
        ok = np.isfinite(inv).all() and np.abs(np.eye(k) - Af @ inv).sum(axis=1).max() < 1e-7
        if ok:
            self.ainv = [[mpf(float(v)) for v in r] for r in np.abs(inv) * (1 + 1e-6)]
        else:
            self.ainv = [absv(r) for r in mp.inverse(mp.matrix(A)).tolist()]
        self.LU = [None] * k
        for i in range(k):
            self.LU[perm[i]] = [mpf(float(v)) for v in LU[i]]
        self.eA = eA or [[mpf(0)] * k for _ in range(k)]

    def __call__(self, b):
        k = self.k
        z = [b[self.perm[i]] for i in range(k)]
        for i in range(k):
            z[i] -= fdot(self.L[i][:i], z[:i])
        for i in reversed(range(k)):
            z[i] = (z[i] - fdot(self.U[i][i + 1:], z[i + 1:])) / self.U[i][i]
        return z


def matvec(H, v):
    return [fdot(row, v) for row in H]


def _check_values(rep, ev, f, g, ks, what):
    class _W:
        def see(self, label, ratio):
            rep.see(label, ratio)
    rep.bad += hp_cases.audit(ev, f, g, ks, "float64", worst=_W(), what=what)


def _step_bound(e, x0, x1, scale=1):
    """scale e_j + the trial point and the stored difference: 3 u (|x_k,j| + |x_k+1,j|)"""
    u, eta = hp_lib.U["float64"], hp_lib.ETA["float64"]
    return [scale * e[j] + 3 * u * (abs(x0[j]) + abs(x1[j])) + 3 * eta for j in range(len(x0))]


def _check_step(rep, s, want, bound, what, note=""):
    for j in range(len(s)):
        err = abs(s[j] - want[j])
        rep.see("direction", err / bound[j])
        if err > bound[j]:
            rep.bad.append("%s coordinate %d: |s - step| = %s, bound %s%s" % (what, j, mp.nstr(err, 5), mp.nstr(bound[j], 5),
                                                                            note))
            return False
    return True


def _shrunk(rho, t):
    """alpha after t successive fl(alpha * rho) from 1, and the one before it"""
    alpha, previous = 1.0, None
    for _ in range(t):
        previous, alpha = alpha, alpha * rho
    return alpha, previous


def _armijo(rep, what, evaluate, ks, x0, f0, f1, d, e_d, cache, e_cache, alpha, previous, promised):
    """the accepted trial meets f_k+1 <= f_k + alpha cache; the trial before it (the definition's value at x_k + alpha_prev d)
    does not"""
    u, eta = hp_lib.U["float64"], hp_lib.ETA["float64"]
    n = len(x0)
    if promised:
        a = mpf(alpha)
        over = f1 - (f0 + a * cache)
        slack = a * e_cache + 2 * u * (abs(f0) + a * abs(cache)) + 2 * eta
        rep.see("armijo", over / slack if over > 0 else 0)
        if over > slack:
            rep.bad.append("%s: the accepted trial misses the Armijo condition by %s, slack %s (alpha = %r)"
                           % (what, mp.nstr(over, 5), mp.nstr(slack, 5), alpha))
    if previous is not None:
        a = mpf(previous)
        trial = [x0[j] + a * d[j] for j in range(n)]
        ev = evaluate(np.array([float(v) for v in trial]))
        moved = [a * e_d[j] + 2 * u * abs(trial[j]) for j in range(n)]
        slack = (a * e_cache + 2 * u * (abs(f0) + a * abs(cache)) + hp_lib.bound(ks[0], ev.f_abs) + fdot(absv(ev.g), moved))
        under = (f0 + a * cache) - ev.f
        rep.see("armijo_before", under / slack if under > 0 else 0)
        if under > slack:
            rep.bad.append("%s: the trial before the accepted one (alpha = %r) meets the Armijo condition by %s, slack %s"
                           % (what, previous, mp.nstr(under, 5), mp.nstr(slack, 5)))


# ---- NewtonDescent -------------------------------------------------------------------------------------------------------------
def audit_newton_descent(xs, gs, fs, dnfev, dsumk, rules, evaluate, ks, what=""):
    """xs, gs [T + 1, n], fs [T + 1], dnfev, dsumk [T]; evaluate(x, hessian=False) -> hp_lib.Eval; ks = (k_f, k_g, k_H)"""
    rep = Report()
    T, n = len(xs) - 1, len(xs[0])
    u, D, cfg = rules.u, rules.depth(n), rules.config
    guard, c = mpf(cfg["safe_guard"]), mpf(cfg["armijo_c"])
    kq = mpf((0.5 * cfg["armijo_c"]) * cfg["armijo_c"])          # the double armijo.h:93 forms, left to right
    rep.iterations = T
    for k in range(T + 1):
        ev = evaluate(xs[k], hessian=k < T)
        tag = "%s iteration %d" % (what, k + 1)
        _check_values(rep, ev, fs[k], gs[k], ks, "%s iterate %d" % (what, k))
        if k == T:
            break
        x0, x1, g = hp_lib.vec(xs[k]), hp_lib.vec(xs[k + 1]), hp_lib.vec(gs[k])
        f0, f1 = mpf(float(fs[k])), mpf(float(fs[k + 1]))
        s = hp_lib.vec(np.asarray(xs[k + 1]) - np.asarray(xs[k]))
        A = [[ev.H[i][j] + (guard if i == j else 0) for j in range(n)] for i in range(n)]
        eA = [[ks[2] * u * ev.H_abs[i][j] + (u * (ev.H_abs[i][i] + guard) if i == j else 0) for j in range(n)]
              for i in range(n)]
        solve = Solve(A, eA)
        d = solve([-v for v in g])
        e_d = solve.error(absv(d), [mpf(0)] * n, u)
        t = int(dsumk[k]) - 1
        if t < 0 or int(dnfev[k]) != t + 4:     # 1 (step) + 1 (the search at x) + the trials + 1 (rebuild)
            rep.bad.append("%s: %d trials and %d evaluations are not a search" % (tag, t + 1, int(dnfev[k])))
            continue
        alpha, previous = _shrunk(cfg["armijo_rho"], t)
        _check_step(rep, s, [mpf(alpha) * v for v in d], _step_bound(e_d, x0, x1, mpf(alpha)), tag,
                    " (alpha = %r after %d trials)" % (alpha, t + 1))
        ad = absv(d)
        Hd_abs = matvec(ev.H_abs, ad)
        gd, dHd = fdot(g, d), fdot(d, matvec(ev.H, d))
        cache = c * gd + kq * dHd
        e_cache = (c * ((D + 2) * u * fdot(absv(g), ad) + fdot(absv(g), e_d))
                   + kq * ((n + D + 2 + ks[2]) * u * fdot(ad, Hd_abs) + 2 * fdot(Hd_abs, e_d)) + u * abs(cache))
        fixed = alpha * cfg["armijo_rho"] == alpha
        rep.no_promise += fixed
        rep.armijo_first += t == 0
        rep.armijo_later += t > 0
        _armijo(rep, tag, evaluate, ks, x0, f0, f1, d, e_d, cache, e_cache, alpha, previous, not fixed)
        rep.audited += 1
    rep.audited_through.append((T, T))
    return rep


# ---- ConjugatedGradientDescent -----------------------------------------------------------------------------------------------------
def audit_conjugated_gradient(xs, gs, fs, dnfev, dsumk, rules, evaluate, ks, what=""):
    rep = Report()
    T, n = len(xs) - 1, len(xs[0])
    u, D, cfg = rules.u, rules.depth(n), rules.config
    c = mpf(cfg["armijo_c"])
    rep.iterations = T
    d = e = None
    for k in range(T + 1):
        ev = evaluate(xs[k])
        tag = "%s iteration %d" % (what, k + 1)
        _check_values(rep, ev, fs[k], gs[k], ks, "%s iterate %d" % (what, k))
        if k == T:
            break
        x0, x1, g = hp_lib.vec(xs[k]), hp_lib.vec(xs[k + 1]), hp_lib.vec(gs[k])
        f0, f1 = mpf(float(fs[k])), mpf(float(fs[k + 1]))
        s = hp_lib.vec(np.asarray(xs[k + 1]) - np.asarray(xs[k]))
        if k == 0:
            d, e = [-v for v in g], [mpf(0)] * n
        else:
            gp = hp_lib.vec(gs[k - 1])
            beta = fdot(g, g) / fdot(gp, gp)
            dn = [-g[j] + beta * d[j] for j in range(n)]
            e = [beta * e[j] + (2 * D + 2) * u * beta * abs(d[j]) + u * abs(dn[j]) for j in range(n)]
            d = dn
        t = int(dsumk[k]) - 1
        if t < 0 or int(dnfev[k]) != t + 4:
            rep.bad.append("%s: %d trials and %d evaluations are not a search" % (tag, t + 1, int(dnfev[k])))
            continue
        alpha, previous = _shrunk(cfg["armijo_rho"], t)
        _check_step(rep, s, [mpf(alpha) * v for v in d], _step_bound(e, x0, x1, mpf(alpha)), tag,
                    " (alpha = %r after %d trials)" % (alpha, t + 1))
        gd = fdot(g, d)
        cache = c * gd
        e_cache = c * ((D + 2) * u * fdot(absv(g), absv(d)) + fdot(absv(g), e)) + u * abs(cache)
        ran_out = not alpha > cfg["armijo_alpha_min"]
        rep.no_promise += ran_out
        rep.armijo_first += t == 0
        rep.armijo_later += t > 0
        _armijo(rep, tag, evaluate, ks, x0, f0, f1, d, e, cache, e_cache, alpha, previous, not ran_out)
        rep.audited += 1
    rep.audited_through.append((T, T))
    return rep


# ---- TrustRegionNewton ---------------------------------------------------------------------------------------------------------------
def _to_boundary(p, e_p, d, e_d, radius, D, u):
    """p + tau d with the positive root of |p + tau d| = radius, and its running bound"""
    n = len(p)
    ap, ad = absv(p), absv(d)
    a = fdot(d, d)
    e_a = D * u * a + 2 * fdot(ad, e_d)
    b = 2 * fdot(p, d)
    e_b = 2 * (D * u * fdot(ap, ad) + fdot(ap, e_d) + fdot(e_p, ad))
    pp, r2 = fdot(p, p), radius * radius
    c = pp - r2
    e_c = D * u * pp + 2 * fdot(ap, e_p) + u * r2 + u * (pp + r2)
    disc = b * b - 4 * a * c
    e_disc = 2 * abs(b) * e_b + u * b * b + 4 * (a * e_c + abs(c) * e_a) + 8 * u * abs(a * c) + u * (b * b + 4 * abs(a * c))
    _decide(disc, e_disc, "the discriminant of the boundary root against 0")
    sq = mp.sqrt(disc)
    e_sq = e_disc / (2 * sq) + u * sq
    num = -b + sq
    e_num = e_b + e_sq + u * abs(num)
    tau = num / (2 * a)
    e_tau = e_num / (2 * a) + abs(tau) * (e_a / a + u)
    pn = [p[j] + tau * d[j] for j in range(n)]
    return pn, [e_p[j] + e_tau * ad[j] + abs(tau) * e_d[j] + u * abs(tau * d[j]) + u * abs(pn[j]) for j in range(n)]


def steihaug(H, H_abs, g, radius, tolerance, e_tolerance, cap, D, u, k_H):
    """CG-Steihaug at 200 bits -> (p, e_p, ended on the boundary, iterations, how it ended); raises Undecidable"""
    n = len(g)
    zero = [mpf(0)] * n
    p, e_p, r, e_r, d, e_d = zero, zero, list(g), zero, [-v for v in g], zero
    rr = fdot(r, r)
    e_rr = D * u * rr
    norm = mp.sqrt(rr)
    _decide(norm - tolerance, (e_rr / (2 * norm) if norm > 0 else 0) + u * norm + e_tolerance, "the early exit")
    if norm <= tolerance:
        return p, e_p, False, 0, "cg_zero"
    for it in range(cap):
        ad = absv(d)
        hd = matvec(H, d)
        e_hd = [(n + k_H) * u * fdot(H_abs[i], ad) + fdot(H_abs[i], e_d) for i in range(n)]
        curvature = fdot(d, hd)
        e_curvature = D * u * fdot(ad, absv(hd)) + fdot(e_d, absv(hd)) + fdot(ad, e_hd)
        _decide(curvature, e_curvature, "the sign of the curvature")
        if not curvature > 0:
            p, e_p = _to_boundary(p, e_p, d, e_d, radius, D, u)
            return p, e_p, True, it + 1, "cg_negative"
        alpha = rr / curvature
        e_alpha = alpha * (e_rr / rr + e_curvature / curvature + u)
        pc = [p[j] + alpha * d[j] for j in range(n)]
        e_pc = [e_p[j] + e_alpha * ad[j] + alpha * e_d[j] + u * abs(alpha * d[j]) + u * abs(pc[j]) for j in range(n)]
        pp = fdot(pc, pc)
        norm = mp.sqrt(pp)
        _decide(norm - radius, (D * u * pp + 2 * fdot(absv(pc), e_pc)) / (2 * norm) + u * norm, "the boundary crossing")
        if norm >= radius:
            p, e_p = _to_boundary(p, e_p, d, e_d, radius, D, u)
            return p, e_p, True, it + 1, "cg_boundary"
        p, e_p = pc, e_pc
        rn = [r[j] + alpha * hd[j] for j in range(n)]
        e_r = [e_r[j] + e_alpha * abs(hd[j]) + alpha * e_hd[j] + u * abs(alpha * hd[j]) + u * abs(rn[j]) for j in range(n)]
        r = rn
        rr_new = fdot(r, r)
        e_rr_new = D * u * rr_new + 2 * fdot(absv(r), e_r)
        norm = mp.sqrt(rr_new)
        _decide(norm - tolerance, (e_rr_new / (2 * norm) if norm > 0 else 0) + u * norm + e_tolerance, "the CG tolerance")
        if norm <= tolerance:
            return p, e_p, False, it + 1, "cg_tolerance"
        beta = rr_new / rr
        e_beta = beta * (e_rr_new / rr_new + e_rr / rr + u)
        dn = [-r[j] + beta * d[j] for j in range(n)]
        e_d = [e_r[j] + e_beta * ad[j] + beta * e_d[j] + u * abs(beta * d[j]) + u * abs(dn[j]) for j in range(n)]
        d, rr, e_rr = dn, rr_new, e_rr_new
    return p, e_p, False, cap, "cg_cap"


def _model(H, g, v):
    return fdot(g, v) + fdot(v, matvec(H, v)) / 2


def audit_trust_region(xs, gs, fs, dnfev, dsumk, rules, evaluate, ks, what=""):
    rep = Report()
    T, n = len(xs) - 1, len(xs[0])
    u, D, cfg = rules.u, rules.depth(n), rules.config
    k_f, k_H = ks[0], ks[2]
    radius = float(cfg["initial_radius"])                    # the working-precision scalar, replayed in double
    accept, low, high = mpf(cfg["acceptance_threshold"]), mpf(cfg["rho_low"]), mpf(cfg["rho_high"])
    cap, limit = max(int(cfg["cg_max_iterations_floor"]), 0), min(max(int(cfg["rejection_retry_limit"]), 0), 1000)
    rep.iterations = T
    alive, through = True, 0
    for k in range(T + 1):
        ev = evaluate(xs[k], hessian=k < T)
        tag = "%s iteration %d" % (what, k + 1)
        _check_values(rep, ev, fs[k], gs[k], ks, "%s iterate %d" % (what, k))
        if k == T:
            break
        H, H_abs = ev.H, ev.H_abs
        x0, x1, g = hp_lib.vec(xs[k]), hp_lib.vec(xs[k + 1]), hp_lib.vec(gs[k])
        ag = absv(g)
        f0, f1 = mpf(float(fs[k])), mpf(float(fs[k + 1]))
        s = hp_lib.vec(np.asarray(xs[k + 1]) - np.asarray(xs[k]))
        moved = any(v != 0 for v in s)
        xround = [3 * u * (abs(x0[j]) + abs(x1[j])) for j in range(n)]
        as_, Hs = absv(s), matvec(H, s)
        Hs_abs = matvec(H_abs, as_)
        local = ((D + 1) * u * fdot(ag, as_) + (n + D + k_H + 1) * u * fdot(as_, Hs_abs) / 2
                 + fdot([abs(g[j] + Hs[j]) for j in range(n)], xround))
        if moved:                                             # on every accepted step, audited or not
            predicted = -_model(H, g, s)
            rep.see("predicted", -predicted / local if predicted < 0 else 0)
            if predicted < -local:
                rep.bad.append("%s: an accepted step with predicted reduction %s, slack %s"
                               % (tag, mp.nstr(predicted, 5), mp.nstr(local, 5)))
        if not alive:
            rep.unaudited += 1
            continue
        try:
            gnorm = max(ag)
            tolerance = mpf(cfg["cg_forcing_coefficient"]) * min(mpf(1) / 2, mp.sqrt(gnorm)) * gnorm
            nfev, sumk, accepted, why_stalled = 1, 0, False, "the retries are exhausted"
            branches = dict.fromkeys(BRANCHES, 0)
            for retry in range(limit):
                used = radius
                p, e_p, hit, iters, how = steihaug(H, H_abs, g, mpf(radius), tolerance, 3 * u * tolerance, cap, D, u, k_H)
                branches[how] += 1
                nfev += 1
                sumk += iters
                ap = absv(p)
                Hp_abs = matvec(H_abs, ap)
                gp, pHp = fdot(g, p), fdot(p, matvec(H, p))
                predicted = -gp - pHp / 2
                e_predicted = (D * u * fdot(ag, ap) + fdot(ag, e_p)
                               + ((n + k_H + D) * u * fdot(ap, Hp_abs) + 2 * fdot(Hp_abs, e_p)) / 2
                               + 2 * u * (abs(gp) + abs(pHp) / 2))
                trial = [x0[j] + p[j] for j in range(n)]
                et = evaluate(np.array([float(v) for v in trial]))
                e_value = hp_lib.bound(k_f, et.f_abs) + fdot(absv(et.g), [e_p[j] + 2 * u * abs(trial[j]) for j in range(n)])
                _decide(predicted, e_predicted, "the sign of the predicted reduction")
                if predicted <= 0:
                    rho, e_rho = -INF, mpf(0)
                else:
                    actual = f0 - et.f
                    rho = actual / predicted
                    e_rho = (e_value + u * abs(actual)) / predicted + abs(rho) * (e_predicted / predicted + u)
                    _decide(rho - accept, e_rho, "rho against the acceptance threshold")
                taken = rho > accept
                if taken:                                     # the device's own f_k+1 from here on
                    actual = f0 - f1
                    rho = actual / predicted
                    e_rho = u * abs(actual) / predicted + abs(rho) * (e_predicted / predicted + u)
                    rep.see("rho", ((accept - rho) / e_rho if e_rho > 0 else INF) if rho < accept else 0)
                    if rho < accept - e_rho:
                        rep.bad.append("%s: rho = %s on the device's own values, below the acceptance threshold" % (tag, mp.nstr(rho, 8)))
                _decide(rho - low, e_rho, "rho against rho_low")
                if rho < low:
                    radius = radius * float(cfg["shrink_factor"])
                    branches["shrinks"] += 1
                elif hit:
                    _decide(rho - high, e_rho, "rho against rho_high")
                    if rho > high:
                        radius = min(float(cfg["expand_factor"]) * radius, float(cfg["max_radius"]))
                        branches["grows"] += 1
                if taken:
                    nfev += 1
                    accepted = True
                    break
                branches["retries"] += 1
                if radius <= float(cfg["min_radius"]):
                    why_stalled = "the radius is at min_radius"
                    break
                if radius == used:                            # every remaining retry repeats this one: counted, not run
                    left = limit - retry - 1
                    nfev += left
                    sumk += left * iters
                    why_stalled = "the radius stays put between rho_low and the acceptance threshold"
                    break
        except Undecidable as reason:
            rep.undecidable.append("%s: %s" % (tag, reason))
            alive = False
            rep.unaudited += 1
            continue
        for b, v in branches.items():
            setattr(rep, b, getattr(rep, b) + v)
        if (nfev, sumk) != (int(dnfev[k]), int(dsumk[k])):
            rep.bad.append("%s: the rules give %d evaluations and %d CG iterations, the solve took %d and %d"
                           % (tag, nfev, sumk, int(dnfev[k]), int(dsumk[k])))
            alive = False
            rep.unaudited += 1
            continue
        if not accepted:
            rep.stalls += 1
            if moved:
                rep.bad.append("%s: x moved where the rules stall (%s)" % (tag, why_stalled))
        elif not moved and any(v != 0 for v in p):
            rep.bad.append("%s: x did not move where the rules accept a step" % tag)
        else:
            _check_step(rep, s, p, _step_bound(e_p, x0, x1), tag, " (radius %r)" % used)
            norm, e_norm = hp_lib.norm2(s), hp_lib.norm2(_step_bound(e_p, x0, x1)) + (D + 2) * u * mpf(used)
            rep.see("radius", (norm - used) / e_norm if norm > used else 0)
            if norm > used + e_norm:
                rep.bad.append("%s: |s| = %s beyond the radius %r" % (tag, mp.nstr(norm, 17), used))
            # Steihaug's guarantee: no worse than the Cauchy point within the radius
            gHg, gg = fdot(g, matvec(H, g)), fdot(g, g)
            tau = mpf(used) / mp.sqrt(gg)
            if gHg > 0:
                tau = min(tau, gg / gHg)
            over = _model(H, g, s) - _model(H, g, [-tau * v for v in g])
            slack = local + fdot([abs(g[j] + Hs[j]) for j in range(n)], e_p)
            rep.see("cauchy", over / slack if over > 0 else 0)
            if over > slack:
                rep.bad.append("%s: the model at s is %s above the model at the Cauchy point, slack %s"
                               % (tag, mp.nstr(over, 5), mp.nstr(slack, 5)))
        rep.audited += 1
        through = k + 1
    rep.audited_through.append((through if not alive else T, T))
    return rep


AUDITS = {"trust_region": audit_trust_region, "newton_descent": audit_newton_descent,
          "conjugated_gradient": audit_conjugated_gradient}


def audit_case(trajectories, rules, evaluate, ks, what=""):
    """trajectories: [(xs, gs, fs, dnfev, dsumk)] of the traced problems of one case -> the merged Report"""
    total = Report()
    for i, (xs, gs, fs, dnfev, dsumk) in enumerate(trajectories):
        tag = "%s problem %d" % (what, i)
        if rules.solver == "gradient_descent":
            rep = Report()
            base = step_lib.audit_problem(xs, gs, fs, rules, what=tag)
            step_lib.audit_values(evaluate, ks[:2], xs, gs, fs, rules.dtype, base, what=tag)
            step_lib.Report.merge(rep, base)
            # The search starts at the step 1 (gradient_descent.h:70, more_thuente.h's alpha_init): where it took one trial
            # (d sum_k = 1) it accepted that step, and s is -g itself, not a fitted multiple: three roundings
            for k in range(len(dsumk)):
                if int(dsumk[k]) == 1:
                    x0, x1 = hp_lib.vec(xs[k]), hp_lib.vec(xs[k + 1])
                    _check_step(rep, hp_lib.vec(np.asarray(xs[k + 1]) - np.asarray(xs[k])), [-v for v in hp_lib.vec(gs[k])],
                                _step_bound([mpf(0)] * len(x0), x0, x1), "%s iteration %d" % (tag, k + 1),
                                " (one trial: the unit step along -g)")
            rep.armijo_first += int(sum(int(v) == 1 for v in dsumk))
            rep.armijo_later += int(sum(int(v) > 1 for v in dsumk))
        else:
            rep = AUDITS[rules.solver](xs, gs, fs, dnfev, dsumk, rules, evaluate, ks, what=tag)
        total.merge(rep)
    return total


# ---- plain generators of each step, as the reference writes it, that can carry planted bugs -----------------------------------
# numpy in double with a pairwise tree for every inner product and an ascending chain for H d.  Without a bug their
# trajectories pass the audit; tests/test_nstep_lib.py plants each bug and shows that the audit sees it.
CG_EARLY = "CG-Steihaug stops one iteration early"
CG_LATE = "CG-Steihaug stops one iteration late"
OTHER_ROOT = "the boundary step takes the other root tau"
GROW_WITHOUT_HIT = "the radius grows without the boundary being hit"
RHO_LINEAR = "rho uses predicted = -g.p only"
STALE_H = "H from x_k-1"
TR_BUGS = (CG_EARLY, CG_LATE, OTHER_ROOT, GROW_WITHOUT_HIT, RHO_LINEAR, STALE_H)
NO_GUARD = "safe_guard left off"
GUARD_EVERYWHERE = "safe_guard added to every entry of H"
NO_CURVATURE = "the curvature term dropped from the cache"
HALF_C = "the curvature term with c / 2 in place of c c / 2"
SHRINK_FIRST = "alpha shrinks before the first trial"
ND_BUGS = (NO_GUARD, GUARD_EVERYWHERE, NO_CURVATURE, HALF_C, SHRINK_FIRST)
BETA_INVERTED = "beta inverted"
BETA_MIXED = "beta from g_k.g_k-1"
ALWAYS_RESET = "d reset to -g every step"
CG_BUGS = (BETA_INVERTED, BETA_MIXED, ALWAYS_RESET)
NORMALISED = "steps along -g normalised"
DECREASE_ALONE = "acceptance on sufficient decrease alone"
GD_BUGS = (NORMALISED, DECREASE_ALONE)
tree_dot = step_lib.tree_dot


def _chain(H, v):
    out = H[:, 0] * v[0]
    for k in range(1, len(v)):
        out = out + H[:, k] * v[k]
    return out


def _done(x, g, gradient_norm):
    return np.max(np.abs(g)) < gradient_norm * max(1.0, np.max(np.abs(x)))


def _pack(xs, gs, fs, dnfev, dsumk):
    return np.array(xs), np.array(gs), np.array(fs), np.array(dnfev), np.array(dsumk)


def generate_trust_region(fun, hess, x0, limit, config=None, gradient_norm=1e-6, bug=None):
    """fun(x) -> (f, g), hess(x) -> H; at most limit + 1 iterations, ended by |g|_inf < gradient_norm max(1, |x|_inf)"""
    cfg = dict(DEFAULTS["trust_region"], **(config or {}))
    x = np.asarray(x0, dtype=np.float64)
    n = x.size
    f, g = fun(x)
    radius = cfg["initial_radius"]
    H_before = None
    xs, gs, fs, dnfev, dsumk = [x], [g], [f], [], []

    def boundary(p, d, radius):
        a, b, c = tree_dot(d, d), 2.0 * tree_dot(p, d), tree_dot(p, p) - radius * radius
        root = np.sqrt(max(b * b - 4.0 * a * c, 0.0))
        tau = ((-b - root) if bug == OTHER_ROOT else (-b + root)) / (2.0 * a)
        return p + tau * d

    def subproblem(H, g, radius, tolerance):
        p, r, d = np.zeros(n), g.copy(), -g
        rr = tree_dot(r, r)
        if np.sqrt(rr) <= tolerance:
            return p, False, 0
        late = False
        for it in range(cfg["cg_max_iterations_floor"]):
            hd = _chain(H, d)
            curvature = tree_dot(d, hd)
            if not curvature > 0:
                return boundary(p, d, radius), True, it + 1
            alpha = rr / curvature
            pc = p + alpha * d
            if np.sqrt(tree_dot(pc, pc)) >= radius:
                return boundary(p, d, radius), True, it + 1
            before = p
            p = pc
            r = r + alpha * hd
            rr_new = tree_dot(r, r)
            if np.sqrt(rr_new) <= tolerance:
                if bug == CG_EARLY and it > 0:
                    return before, False, it
                if bug != CG_LATE or late:
                    return p, False, it + 1
                late = True
            elif late:
                return p, False, it + 1
            d = -r + (rr_new / rr) * d
            rr = rr_new
        return p, False, cfg["cg_max_iterations_floor"]

    for _ in range(limit + 1):
        H = hess(x)
        model_H = H_before if (bug == STALE_H and H_before is not None) else H
        H_before = H
        gnorm = np.max(np.abs(g))
        tolerance = cfg["cg_forcing_coefficient"] * min(0.5, np.sqrt(gnorm)) * gnorm
        nfev, sumk, taken = 1, 0, False
        for retry in range(cfg["rejection_retry_limit"]):
            p, hit, iters = subproblem(model_H, g, radius, tolerance)
            sumk += iters
            xt = x + p
            ft, gt = fun(xt)
            nfev += 1
            predicted = -tree_dot(g, p) - (0.0 if bug == RHO_LINEAR else 0.5 * tree_dot(p, _chain(model_H, p)))
            rho = -np.inf if predicted <= 0 else (f - ft) / predicted
            used = radius
            if rho < cfg["rho_low"]:
                radius = radius * cfg["shrink_factor"]
            elif rho > cfg["rho_high"] and (hit or bug == GROW_WITHOUT_HIT):
                radius = min(cfg["expand_factor"] * radius, cfg["max_radius"])
            if rho > cfg["acceptance_threshold"]:
                x, f, g = xt, ft, gt
                nfev += 1
                taken = True
                break
            if radius <= cfg["min_radius"]:
                break
            if radius == used:
                left = cfg["rejection_retry_limit"] - retry - 1
                nfev += left
                sumk += left * iters
                break
        xs.append(x)
        gs.append(g)
        fs.append(f)
        dnfev.append(nfev)
        dsumk.append(sumk)
        if _done(x, g, gradient_norm) or not taken:
            break
    return _pack(xs, gs, fs, dnfev, dsumk)


def _backtrack(fun, x, f, d, cache, rho, alpha, stop):
    ft, gt = fun(x + alpha * d)
    trials = 1
    while ft > f + alpha * cache and not stop(alpha):
        alpha = alpha * rho
        ft, gt = fun(x + alpha * d)
        trials += 1
    return x + alpha * d, ft, gt, trials


def generate_newton_descent(fun, hess, x0, limit, config=None, gradient_norm=1e-6, bug=None):
    cfg = dict(DEFAULTS["newton_descent"], **(config or {}))
    c, rho = cfg["armijo_c"], cfg["armijo_rho"]
    x = np.asarray(x0, dtype=np.float64)
    n = x.size
    f, g = fun(x)
    xs, gs, fs, dnfev, dsumk = [x], [g], [f], [], []
    for _ in range(limit + 1):
        H = hess(x)
        A = H.copy()
        if bug == GUARD_EVERYWHERE:
            A = A + cfg["safe_guard"]
        elif bug != NO_GUARD:
            A[np.arange(n), np.arange(n)] += cfg["safe_guard"]
        d = np.linalg.solve(A, -g)
        curvature = tree_dot(_chain(H.T, ((0.5 * c) if bug == HALF_C else ((0.5 * c) * c)) * d), d)
        cache = c * tree_dot(g, d) + (0.0 if bug == NO_CURVATURE else curvature)
        x, f, g, trials = _backtrack(fun, x, f, d, cache, rho, rho if bug == SHRINK_FIRST else 1.0, lambda a: a * rho == a)
        xs.append(x)
        gs.append(g)
        fs.append(f)
        dnfev.append(trials + 3)
        dsumk.append(trials)
        if _done(x, g, gradient_norm):
            break
    return _pack(xs, gs, fs, dnfev, dsumk)


def generate_conjugated_gradient(fun, x0, limit, config=None, gradient_norm=1e-6, bug=None):
    cfg = dict(DEFAULTS["conjugated_gradient"], **(config or {}))
    x = np.asarray(x0, dtype=np.float64)
    f, g = fun(x)
    d = g_before = None
    xs, gs, fs, dnfev, dsumk = [x], [g], [f], [], []
    for _ in range(limit + 1):
        if d is None or bug == ALWAYS_RESET:
            d = -g
        else:
            top, bottom = tree_dot(g, g), tree_dot(g_before, g_before)
            if bug == BETA_MIXED:
                top = tree_dot(g, g_before)
            beta = bottom / top if bug == BETA_INVERTED else top / bottom
            d = (-g) + (beta * d)
        g_before = g
        cache = cfg["armijo_c"] * tree_dot(g, d)
        x, f, g, trials = _backtrack(fun, x, f, d, cache, cfg["armijo_rho"], 1.0,
                                     lambda a: not a > cfg["armijo_alpha_min"])
        xs.append(x)
        gs.append(g)
        fs.append(f)
        dnfev.append(trials + 3)
        dsumk.append(trials)
        if _done(x, g, gradient_norm):
            break
    return _pack(xs, gs, fs, dnfev, dsumk)


def generate_gradient_descent(fun, x0, limit, gradient_norm=1e-6, bug=None):
    """steepest descent from alpha = 1 under the bracketing search of step_lib.generate for the strong Wolfe conditions
    (1e-4, 0.9): bisection inside a bracket, times four before one — NOT More-Thuente's interpolation as the reference
    writes it.  The audit holds a step to the conditions and, where the first trial is accepted, to the unit step; any
    search that meets them from alpha = 1 serves."""
    x = np.asarray(x0, dtype=np.float64)
    f, g = fun(x)
    xs, gs, fs, dnfev, dsumk = [x], [g], [f], [], []
    for _ in range(limit + 1):
        d = -g / np.sqrt(tree_dot(g, g)) if bug == NORMALISED else -g
        slope0 = tree_dot(g, d)
        step, low, high = 1.0, 0.0, None
        for trials in range(1, 61):
            xn = x + step * d
            fn, gn = fun(xn)
            slope = tree_dot(gn, d)
            if not fn <= f + 1e-4 * step * slope0:
                high = step
            elif bug == DECREASE_ALONE or abs(slope) <= 0.9 * (-slope0):
                break
            elif slope < 0:
                low = step
            else:
                high = step
            step = (low + high) / 2.0 if high is not None else step * 4.0
        x, f, g = xn, fn, gn
        xs.append(x)
        gs.append(g)
        fs.append(f)
        dnfev.append(trials + 3)
        dsumk.append(trials)
        if _done(x, g, gradient_norm):
            break
    return _pack(xs, gs, fs, dnfev, dsumk)
