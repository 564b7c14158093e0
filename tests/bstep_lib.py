"""Every iterate of an L-BFGS-B solve against the textbook definition of the step that produced it, at 200 bits.

TEST INFRASTRUCTURE.  mpmath only (the context of tests/hp_lib.py), with the Rules, the Report base and the two caps of
tests/step_lib.py: nothing here comes from oracle/, from the package or from the reference tree.  Inputs are the exact doubles
of a trajectory x_0 .. x_T, g_0 .. g_T and the box.

The rules of the reference's `Lbfgsb::OptimizationStep` (solver/lbfgsb.h), restated:
  pairs    s = fl(x_{k+1} - x), y = fl(g_{k+1} - g) in the working precision; stored iff s^T y > 1e-7 y^T y (:211); the ring
           holds m columns and loses its oldest; theta = y^T y / y^T s of the newest STORED pair, 1 before any.
  B_k      the direct BFGS update B - (B s)(B s)^T / s^T B s + y y^T / y^T s from theta I over the stored pairs, oldest to
           newest — never theta I - W M W^T.  Up to DENSE_MAX a matrix; above it the same operator through the unrolled
           products b_i = B_i s_i (O(p^2 n)).
  Cauchy   the first local minimiser of m(z) = g^T z + z^T B z / 2 along x(t) = P(x - t g): on every segment
           f' = g^T d + d^T B z and f'' = d^T B d from B itself.  Quirks as rules: a coordinate with t_j = 0 has d_j = 0 and
           does not drift; g_j = 0 means t_j = max; f'' is floored at 1e-12 on entry and at 1e-12 f''_0 in the loop; the loop
           goes on while dt_min >= dt; the last dt_min is max(dt_min, 0); a coordinate pinned in the loop sits exactly on its
           bound (:416-427).  Breakpoints that tie are crossed together (the order cannot change the result).
  free     the coordinates not pinned in the loop whose Cauchy value is not a bound (:463-468).
  subspace du solves (Z^T B Z) du = -Z^T (g + B z): a dense solve up to DENSE_MAX; above it through the 2p x 2p Woodbury
           systems, proved by its residual against the unrolled B to 1e-40 (tests/test_bstep_lib.py holds the two routes to
           each other).
  alpha*   `FindAlpha`, with its skip of |du_i| < 1e-7; d = z + alpha* du on the free coordinates, z elsewhere.
  step     with a free variable x_{k+1} = P(x + t d) for one t > 0, fitted on the coordinates that are not on a bound at
           x_{k+1}; a coordinate on a bound there must have x_j + t d_j at or beyond it.  (x_{k+1} = x exactly: the search
           returned its start, a line-search exception under the cap.)  With no free variable x_{k+1} is the
           Cauchy point: t = 1, nothing is fitted (:191-193).

The bound, per coordinate, is that of tests/step_lib.py: |s_j - t d_j| <= t e_j + 3 u (|x_j| + |x_k+1,j|) + the derived term
of the fitted t, where e_j = K u A_j is a RUNNING first-order bound carried through the objects any implementation of the
paper solves with, each evaluated at 200 bits (the VALUE of d comes from the dense definition above; only the sensitivity
from the compact form W = [Y  theta S], MM = [[-D, L^T], [L, theta S^T S]], N = I - MM^-1 W_Z^T W_Z / theta):
  every inner product  D u against the product of absolute values (D: `Rules.depth`);
  every solve          |A^-1| (e_b + (3 * 2p u |L||U| + e_A) |A^-1| |b|): Skeel's componentwise form, with |L||U| of the
                       partially pivoted factorisation at 200 bits — the growth is in the companion, not in a constant;
  f', f''              K_f u against their companions (d_0 in place of d, t |d_0| in place of z), K_f = 2 D + 8 p + 3 on entry
                       and D + 8 p + 12 more per breakpoint crossed (`cauchy_K`); the relative error of dt_min is theirs;
  theta, MM, W         the cancelling sums behind them enter whole (D u |s|^T|y| / s^T y), as rho and gamma do in step_lib.
Nothing is fitted: there is no second constant ("The L-BFGS-B step as a definition").

A decision (dt_min >= dt, a floor, the free test, the 1e-7 skip where it would bind, the pair rule) is UNDECIDABLE when its
200-bit margin is inside the counted slack of what it compares; that problem's audit ends there.
"""
import numpy as np

import hp_lib
import step_lib
from hp_lib import mp, mpf
from step_lib import absv, fdot

DENSE_MAX = 17
FLOOR = mpf(1e-12)          # lbfgsb.h:324
SKIP = mpf(1e-7)            # lbfgsb.h:442
PAIR = mpf(1e-7)            # lbfgsb.h:211
INF = mpf("inf")
Rules = step_lib.Rules


# ---- B_k from the definition --------------------------------------------------------------------------------------------------
class Model:
    """B_k: the direct BFGS update from theta I over `pairs` [(s, y)] oldest first."""

    def __init__(self, pairs, theta, n, dense=None):
        self.n, self.theta, self.pairs = n, theta, pairs
        self.dense = (n <= DENSE_MAX) if dense is None else dense
        self.terms = []                                  # (b_i, s_i^T b_i, y_i, y_i^T s_i)
        for s, y in pairs:
            b = self._unrolled(s)
            self.terms.append((b, fdot(s, b), y, fdot(y, s)))
        self.matrix = None
        if self.dense:
            B = [[theta if i == j else mpf(0) for j in range(n)] for i in range(n)]
            for s, y in pairs:
                b = [fdot(row, s) for row in B]
                sb, ys = fdot(s, b), fdot(y, s)
                B = [[B[i][j] - b[i] * b[j] / sb + y[i] * y[j] / ys for j in range(n)] for i in range(n)]
            self.matrix = B

    def _unrolled(self, v):
        out = [self.theta * e for e in v]
        for b, sb, y, ys in self.terms:
            cb, cy = fdot(b, v) / sb, fdot(y, v) / ys
            out = [out[j] - cb * b[j] + cy * y[j] for j in range(self.n)]
        return out

    def apply(self, v, dense=None):
        if self.dense if dense is None else dense:
            return [fdot(row, v) for row in self.matrix]
        return self._unrolled(v)


def _lu(A):
    """partial pivoting at 200 bits -> (perm, L, U), A[perm[i]] = (L U)[i]"""
    k = len(A)
    A = [row[:] for row in A]
    perm = list(range(k))
    L = [[mpf(0)] * k for _ in range(k)]
    for c in range(k):
        piv = max(range(c, k), key=lambda r: abs(A[r][c]))
        A[c], A[piv], perm[c], perm[piv] = A[piv], A[c], perm[piv], perm[c]
        L[c], L[piv] = L[piv], L[c]
        L[c][c] = mpf(1)
        for r in range(c + 1, k):
            L[r][c] = A[r][c] / A[c][c]
            A[r] = [A[r][j] - L[r][c] * A[c][j] if j >= c else mpf(0) for j in range(k)]
    return perm, L, A


class Solve:
    """A square system at 200 bits with what its rounding error is carried through: |A^-1| and |L||U| (rows in A's order)"""

    def __init__(self, A, eA=None):
        k = self.k = len(A)
        self.A = A
        self.inv = mp.inverse(mp.matrix(A)).tolist() if k else []
        self.ainv = [absv(r) for r in self.inv]
        perm, L, U = _lu(A)
        self.LU = [None] * k
        for i in range(k):
            self.LU[perm[i]] = [sum(abs(L[i][q]) * abs(U[q][j]) for q in range(k)) for j in range(k)]
        self.eA = eA or [[mpf(0)] * k for _ in range(k)]

    def __call__(self, b):
        return [fdot(r, b) for r in self.inv]

    def companion(self, ab):
        return [fdot(r, ab) for r in self.ainv]

    def error(self, ax, eb, u):
        """|dx| <= |A^-1| (e_b + (3 k u |L||U| + e_A) |x|), |x| <= ax"""
        k = self.k
        rhs = [eb[i] + fdot([3 * k * u * self.LU[i][j] + self.eA[i][j] for j in range(k)], ax) for i in range(k)]
        return [fdot(r, rhs) for r in self.ainv]


class Compact:
    """W, MM of the stored pairs at 200 bits, with the entrywise rounding they carry in working precision"""

    def __init__(self, pairs, theta, n, D, u):
        p = self.p = len(pairs)
        self.theta, self.n = theta, n
        S, Y = [q[0] for q in pairs], [q[1] for q in pairs]
        if p:
            s, y = pairs[-1]
            self.etheta = D * u * (1 + fdot(absv(s), absv(y)) / fdot(s, y)) + u     # relative
        else:
            self.etheta = mpf(0)
        self.W = [[Y[i][j] for i in range(p)] + [theta * S[i][j] for i in range(p)] for j in range(n)]
        self.aW = [absv(r) for r in self.W]
        MM = [[mpf(0)] * (2 * p) for _ in range(2 * p)]
        eMM = [[mpf(0)] * (2 * p) for _ in range(2 * p)]
        for i in range(p):
            for j in range(p):
                sy, say = fdot(S[i], Y[j]), fdot(absv(S[i]), absv(Y[j]))
                if i == j:
                    MM[i][i], eMM[i][i] = -sy, D * u * say
                elif i > j:
                    MM[p + i][j] = MM[j][p + i] = sy
                    eMM[p + i][j] = eMM[j][p + i] = D * u * say
                MM[p + i][p + j] = theta * fdot(S[i], S[j])
                eMM[p + i][p + j] = ((D + 1) * u + self.etheta) * theta * fdot(absv(S[i]), absv(S[j]))
        self.M = Solve(MM, eMM)

    def wt(self, v):            # W^T v
        return [fdot([self.W[j][q] for j in range(self.n)], v) for q in range(2 * self.p)]

    def awt(self, av):          # |W|^T |v|
        return [fdot([self.aW[j][q] for j in range(self.n)], av) for q in range(2 * self.p)]


def cauchy_K(p, D, crossed):
    """rounded operations behind f' and f'': on entry d.d (D), theta f' (2), p = W^T d (D), the solve (3 * 2p), its product
    (2p + 1); per breakpoint crossed c + dt p (2) behind W^T z (D), the solve and product again (8 p), and the twelve
    scalar operations of the two updates (:396-401)"""
    return 2 * D + 8 * p + 3 + crossed * (D + 8 * p + 12)


# ---- one step ---------------------------------------------------------------------------------------------------------------
class Step:
    pass


class Undecidable(Exception):
    pass


def breakpoints(x, g, lo, hi):
    out = []
    for j in range(len(x)):
        if g[j] == 0:
            out.append(INF)
        elif g[j] < 0:
            out.append((x[j] - hi[j]) / g[j])
        else:
            out.append((x[j] - lo[j]) / g[j])
    return out


def replay_step(x, g, lo, hi, pairs, theta, rules, dense=None, bounds=True):
    """x, g, lo, hi: lists of mpf; pairs [(s, y)] oldest first.  Returns a Step with z, free, du, alpha, d (the definition)
    and e_d (the running bound on a working-precision d); raises Undecidable."""
    n, p, u = len(x), len(pairs), rules.u
    D = rules.depth(n)
    B = Model(pairs, theta, n, dense)
    cf = Compact(pairs, theta, n, D, u) if bounds else None
    st = Step()
    st.p, st.model = p, B
    tj = breakpoints(x, g, lo, hi)
    d0 = [-g[j] if tj[j] > 0 else mpf(0) for j in range(n)]
    ad0 = absv(d0)
    d = d0[:]
    z = [mpf(0)] * n
    pinned = set()
    groups = sorted({t for t in tj if t > 0 and t != INF})
    t_old, crossed = mpf(0), 0

    def errors(t_here, crossed):
        """the counted slack of f' and f'' on the segment that starts at t_here"""
        if not bounds:
            return mpf(0), mpf(0)
        K = cauchy_K(p, D, crossed)
        zmax = [t_here * e for e in ad0]
        rel = K * u + 2 * cf.etheta
        fp_abs = fdot(ad0, ad0) + theta * fdot(ad0, zmax)
        fpp_abs = theta * fdot(ad0, ad0)
        efp = efpp = mpf(0)
        if p:
            awd, awz = cf.awt(ad0), cf.awt(zmax)
            mwz, mwd = cf.M.companion(awz), cf.M.companion(awd)
            fp_abs += fdot(awd, mwz)
            fpp_abs += fdot(awd, mwd)
            zero = [mpf(0)] * (2 * p)
            efp = fdot(awd, cf.M.error(mwz, zero, u))
            efpp = fdot(awd, cf.M.error(mwd, zero, u))
        return rel * fp_abs + efp, rel * fpp_abs + efpp

    def derivatives():
        Bz = B.apply(z) if crossed or t_old else [mpf(0)] * n
        return fdot(g, d) + fdot(d, Bz), fdot(d, B.apply(d))

    fp, fpp = derivatives()
    efp, efpp = errors(t_old, 0)
    if abs(fpp - FLOOR) <= efpp and fpp != FLOOR:
        raise Undecidable("f'' = %s against its floor" % mp.nstr(fpp, 5))
    fpp = max(FLOOR, fpp)
    fpp0 = fpp
    for t in groups:
        dt_min, dt = -fp / fpp, t - t_old
        slack = efp / fpp + abs(dt_min) * (efpp / fpp + u) + 2 * u * t
        if abs(dt_min - dt) <= slack:
            raise Undecidable("dt_min = %s against dt = %s, slack %s" % (mp.nstr(dt_min, 8), mp.nstr(dt, 8), mp.nstr(slack, 3)))
        if dt_min < dt:
            break
        for j in range(n):
            if tj[j] == t:
                z[j] = (hi[j] if d0[j] > 0 else lo[j]) - x[j]
                d[j] = mpf(0)
                pinned.add(j)
                crossed += 1
        t_old = t
        for j in range(n):
            if j not in pinned:
                z[j] = t_old * d[j]
        if not any(e != 0 for e in d):
            fp, fpp = mpf(0), fpp0
            break
        fp, fpp = derivatives()
        efp, efpp = errors(t_old, crossed)
        floor = FLOOR * fpp0
        if abs(fpp - floor) <= efpp + 2 * u * floor:
            raise Undecidable("f'' = %s against its floor %s" % (mp.nstr(fpp, 5), mp.nstr(floor, 5)))
        fpp = max(floor, fpp)
    dt_min = -fp / fpp
    e_dt = efp / fpp + abs(dt_min) * (efpp / fpp + u)
    dt_min = max(dt_min, mpf(0))          # (continuous: no decision)
    t_tot = t_old + dt_min
    e_t = e_dt + 2 * u * t_tot
    for j in range(n):
        if j not in pinned:
            z[j] = t_tot * d[j]
    ez = [u * abs(z[j]) if j in pinned else ((e_t * abs(d[j]) + 3 * u * abs(z[j]) + 2 * u * abs(x[j])) if d[j] != 0 else mpf(0))
          for j in range(n)]
    st.crossed, st.t, st.z, st.pinned = crossed, t_tot, z, pinned
    # ---- the free set ---------------------------------------------------------------------------------------------------------
    free = []
    for j in range(n):
        if j in pinned:
            continue
        xc = x[j] + z[j]
        for bound in (lo[j], hi[j]):
            if xc != bound and abs(xc - bound) <= ez[j] + 2 * u * abs(xc):
                raise Undecidable("Cauchy value of coordinate %d within %s of its bound" % (j, mp.nstr(abs(xc - bound), 3)))
        if xc != lo[j] and xc != hi[j]:
            free.append(j)
    st.free = free
    st.du, st.alpha = [], mpf(1)
    if not free:
        st.d, st.e_d = z, ez
        return st
    # ---- the subspace step ------------------------------------------------------------------------------------------------------
    Bz = B.apply(z)
    r = [g[j] + Bz[j] for j in free]
    if B.dense:
        H = mp.matrix([[B.matrix[i][j] for j in free] for i in free])
        du = list(mp.lu_solve(H, mp.matrix([-e for e in r])))
    else:
        du = woodbury(pairs, theta, free, r)
        res = subspace_residual(B, free, r, du)
        assert res <= mpf(10) ** -40, "the Woodbury route leaves a residual of %s" % mp.nstr(res, 5)
    st.du = du
    # the bound on du through the compact form
    nf = len(free)
    if not bounds:
        edu = [mpf(0)] * nf
    elif p == 0:
        edu = [(u * (abs(g[j]) + theta * abs(z[j])) + theta * ez[j]) / theta + 2 * u * abs(du[i]) for i, j in enumerate(free)]
    else:
        et, k2 = cf.etheta, 2 * p
        M = cf.M
        awz = cf.awt(absv(z))
        ec = [a + b for a, b in zip(cf.awt(ez), [((D + 2 * crossed + 2) * u + et) * e for e in awz])]
        amc = M.companion(awz)
        emc = M.error(amc, ec, u)
        ar = [abs(g[j]) + theta * abs(z[j]) + fdot(cf.aW[j], amc) for j in free]
        er = [(k2 + 4) * u * ar[i] + theta * ez[j] + et * (theta * abs(z[j]) + fdot(cf.aW[j], amc)) + fdot(cf.aW[j], emc)
              for i, j in enumerate(free)]
        Df = hp_lib.log2_ceil(nf) + (D - hp_lib.log2_ceil(n)) if rules.dot != "sequential" else nf
        aa = [fdot([cf.aW[j][q] for j in free], ar) for q in range(k2)]
        ea = [fdot([cf.aW[j][q] for j in free], er) + ((Df + 1) * u + et) * aa[q] for q in range(k2)]
        av1 = M.companion(aa)
        ev1 = M.error(av1, ea, u)
        K = [[fdot([cf.W[j][a] for j in free], [cf.W[j][b] for j in free]) / theta for b in range(k2)] for a in range(k2)]
        aK = [[fdot([cf.aW[j][a] for j in free], [cf.aW[j][b] for j in free]) / theta for b in range(k2)] for a in range(k2)]
        cols = []
        for b in range(k2):
            col, acol = [K[a][b] for a in range(k2)], [aK[a][b] for a in range(k2)]
            amk = M.companion(acol)
            emk = M.error(amk, [((Df + 2) * u + 3 * et) * e for e in acol], u)
            cols.append((M(col), emk))
        N = [[(1 if a == b else 0) - cols[b][0][a] for b in range(k2)] for a in range(k2)]
        eN = [[cols[b][1][a] + u * abs(N[a][b]) for b in range(k2)] for a in range(k2)]
        Ns = Solve(N, eN)
        av2 = Ns.companion(av1)
        ev2 = Ns.error(av2, ev1, u)
        adu = [ar[i] / theta + fdot(cf.aW[j], av2) / theta ** 2 for i, j in enumerate(free)]
        edu = [er[i] / theta + fdot(cf.aW[j], ev2) / theta ** 2 + ((k2 + 4) * u + 3 * et) * adu[i] for i, j in enumerate(free)]
    # ---- alpha* -----------------------------------------------------------------------------------------------------------------
    def ratio(i):
        j = free[i]
        return ((hi[j] if du[i] > 0 else lo[j]) - (x[j] + z[j])) / du[i]

    alpha, binding = mpf(1), None
    for i in range(nf):
        if abs(du[i]) >= SKIP and ratio(i) < alpha:
            alpha, binding = ratio(i), i
    for i in range(nf):         # the skip is a decision only where the coordinate would bind
        if abs(abs(du[i]) - SKIP) <= edu[i] and du[i] != 0 and ratio(i) < alpha and abs(du[i]) != SKIP:
            raise Undecidable("|du| = %s of coordinate %d against 1e-7" % (mp.nstr(du[i], 8), free[i]))
    ealpha = mpf(0)
    if binding is not None:
        j = free[binding]
        gap = abs((hi[j] if du[binding] > 0 else lo[j]) - (x[j] + z[j]))
        ealpha = alpha * (edu[binding] / abs(du[binding]) + 2 * u) + (ez[j] + 2 * u * abs(x[j] + z[j])) / abs(du[binding])
    st.alpha = alpha
    dvec, e_d = z[:], ez[:]
    for i, j in enumerate(free):
        dvec[j] = z[j] + alpha * du[i]
        e_d[j] = ez[j] + alpha * edu[i] + abs(du[i]) * ealpha + 2 * u * (abs(z[j]) + alpha * abs(du[i]) + abs(x[j]))
    st.d, st.e_d = dvec, e_d
    return st


def woodbury(pairs, theta, free, r):
    """du = -r / theta - W_Z^T (I - MM^-1 W_Z W_Z^T / theta)^-1 MM^-1 W_Z r / theta^2 at 200 bits (exact data: no bound)"""
    p = len(pairs)
    if p == 0:
        return [-e / theta for e in r]
    cf = Compact(pairs, theta, max(free) + 1, 0, mpf(0))
    k2 = 2 * p
    WZ = [[cf.W[j][q] for j in free] for q in range(k2)]
    v = cf.M([fdot(row, r) for row in WZ])
    K = [[fdot(WZ[a], WZ[b]) / theta for b in range(k2)] for a in range(k2)]
    MK = [cf.M([K[a][b] for a in range(k2)]) for b in range(k2)]          # columns
    N = mp.matrix([[(1 if a == b else 0) - MK[b][a] for b in range(k2)] for a in range(k2)])
    v = list(mp.lu_solve(N, mp.matrix(v)))
    return [-r[i] / theta - fdot([WZ[q][i] for q in range(k2)], v) / theta ** 2 for i in range(len(free))]


def subspace_residual(B, free, r, du, dense=None):
    """|| Z^T B Z du + r ||_inf / ||r||_inf against the model's own products"""
    full = [mpf(0)] * B.n
    for i, j in enumerate(free):
        full[j] = du[i]
    Bd = B.apply(full, dense)
    scale = max([abs(e) for e in r] + [mpf(10) ** -300])
    return max(abs(Bd[j] + r[i]) for i, j in enumerate(free)) / scale


# ---- the audit ----------------------------------------------------------------------------------------------------------------
class Report(step_lib.Report):
    COUNTS = ("crossed_with_history", "two_crossed_and_free", "alpha_below_one", "no_free_with_history", "none_crossed")

    def __init__(self):
        super().__init__()
        for k in self.COUNTS:
            setattr(self, k, 0)

    def merge(self, other):
        super().merge(other)
        for k in self.COUNTS:
            setattr(self, k, getattr(self, k) + getattr(other, k))

    def counts(self):
        return tuple(getattr(self, k) for k in self.COUNTS) + (self.rejected,)

    def line(self):
        return ("%d iterations, %d audited, %d unaudited, %d exceptions, (a) %d (b) %d (c) %d (d) %d (e) %d (f) %d, %d evictions, worst %s"
                % ((self.iterations, self.audited, self.unaudited, self.exceptions) + self.counts()
                   + (self.evictions, ", ".join("%s %.3g" % kv for kv in sorted(self.worst.items())))))


caps = step_lib.caps


def audit_problem(xs, gs, rules, what="", keep=None):
    """xs, gs [T + 1, n] of one problem in double; rules.lower, rules.upper its box.  `keep`: a list that receives the Step of
    every audited iteration."""
    rep = Report()
    T, n = len(xs) - 1, len(xs[0])
    u, m = rules.u, rules.m
    D = rules.depth(n)
    lo, hi = hp_lib.vec(np.broadcast_to(rules.lower, (n,))), hp_lib.vec(np.broadcast_to(rules.upper, (n,)))
    X, G = [hp_lib.vec(x) for x in xs], [hp_lib.vec(g) for g in gs]
    ring, theta = [], mpf(1)
    rep.iterations = T
    through = 0
    for k in range(T):
        where = "%s iteration %d" % (what, k + 1)
        x, g = X[k], G[k]
        if not all(lo[j] <= X[k + 1][j] <= hi[j] for j in range(n)):
            rep.bad.append("%s: an iterate outside its box" % where)
        try:
            st = replay_step(x, g, lo, hi, ring, theta, rules)
        except Undecidable as why:
            rep.undecidable.append("%s: %s" % (where, why))
            break
        if keep is not None:
            keep.append(st)
        s = hp_lib.vec(np.asarray(xs[k + 1], dtype=np.float64) - np.asarray(xs[k], dtype=np.float64))
        y = hp_lib.vec(np.asarray(gs[k + 1], dtype=np.float64) - np.asarray(gs[k], dtype=np.float64))
        d, e_d = st.d, st.e_d
        rounding = [3 * u * (abs(x[j]) + abs(X[k + 1][j])) + 3 * hp_lib.ETA[rules.dtype] for j in range(n)]
        if not st.free:
            t, fit, inside = mpf(1), mpf(0), list(range(n))
        else:
            inside = [j for j in range(n) if X[k + 1][j] != lo[j] and X[k + 1][j] != hi[j]]
            dd = fdot([d[j] for j in inside], [d[j] for j in inside])
            t = fdot([s[j] for j in inside], [d[j] for j in inside]) / dd if dd > 0 else None
            if t is not None and t == 0 and all(e == 0 for e in s):
                # the search returned its start: near the end of a run the decrease along d is below the rounding of f and
                # no trial shows it — a line-search exception as in tests/step_lib.py, under the same cap
                rep.exceptions += 1
                rep.exception_notes.append("%s: the search returned its start" % where)
                t = None
            if t is not None and not t > 0:
                rep.bad.append("%s: the step is no positive multiple of d (t = %s)" % (where, mp.nstr(t, 5)))
                t = None
            if t is not None:
                fit = fdot([t * e_d[j] + rounding[j] for j in inside], [abs(d[j]) for j in inside]) / dd
        if t is not None:
            for j in range(n):
                bound = t * e_d[j] + rounding[j] + fit * abs(d[j])
                target = x[j] + t * d[j]
                if j in inside:
                    err = abs(s[j] - t * d[j])
                elif X[k + 1][j] == hi[j]:
                    err = max(mpf(0), hi[j] - target)
                else:
                    err = max(mpf(0), target - lo[j])
                ratio = err / bound if bound > 0 else (mpf(0) if err == 0 else INF)
                rep.see("step", ratio)
                if err > bound:
                    rep.bad.append("%s coordinate %d: |s - t d| = %s, bound %s (t = %s, %d pairs, %d crossed, %d free, alpha* %s)"
                                   % (where, j, mp.nstr(err, 5), mp.nstr(bound, 5), mp.nstr(t, 5), st.p, st.crossed,
                                      len(st.free), mp.nstr(st.alpha, 5)))
                    break
        rep.audited += 1
        through = k + 1
        rep.crossed_with_history += st.crossed >= 1 and st.p >= 1
        rep.two_crossed_and_free += st.crossed >= 2 and len(st.free) >= 1
        rep.alpha_below_one += bool(st.free) and st.alpha < 1
        rep.no_free_with_history += (not st.free) and st.p >= 1
        rep.none_crossed += st.crossed == 0
        # ---- the state after the step ---------------------------------------------------------------------------------------
        sy, yy = fdot(s, y), fdot(y, y)
        slack = D * u * (fdot(absv(s), absv(y)) + PAIR * yy) + 2 * u * PAIR * yy
        if abs(sy - PAIR * yy) <= slack and not (sy == 0 and yy == 0):
            if k + 1 < T:
                rep.undecidable.append("%s: s^T y = %s against 1e-7 y^T y = %s" % (where, mp.nstr(sy, 5), mp.nstr(PAIR * yy, 5)))
            break
        if sy > PAIR * yy:
            if len(ring) == m:
                ring = ring[1:]
                rep.evictions += 1
            ring = ring + [(s, y)]
            theta = yy / sy
        else:
            rep.rejected += 1
    rep.unaudited = T - through
    rep.audited_through.append((through, T))
    return rep


def audit_case(trajectories, rules_of_problem, what=""):
    """trajectories [(xs, gs, fs)], rules_of_problem(i) -> Rules with that problem's box -> the merged Report"""
    total = Report()
    for i, (xs, gs, _) in enumerate(trajectories):
        total.merge(audit_problem(xs, gs, rules_of_problem(i), what="%s problem %d" % (what, i)))
    return total


# ---- a plain trajectory generator that can carry planted bugs ----------------------------------------------------------------------
# Written from the paper (Byrd, Lu, Nocedal, Zhu 1995: algorithm CP and the direct primal method, with B = theta I - W M W^T,
# W = [Y  theta S], M = [[-D, L^T], [L, theta S^T S]]^-1), in numpy doubles with step_lib's pairwise tree for the inner
# products over n, under step_lib.generate's bracketing search from the unit step.
OUT_OF_ORDER = "the breakpoints are visited out of order after the first"
NO_CROSS_TERM = "the 2 g_b w_b^T M p term of f'' is dropped"
C_NOT_ADVANCED = "c is not advanced by the last dt_min p"
W_WITHOUT_THETA = "W is built as [Y S] with no theta on S"
THETA_OLDEST = "theta is taken from the oldest pair"
PAPER_SIGN = "the paper's uncorrected sign in du"
ALPHA_NO_LOWER = "FindAlpha ignores lower bounds"
FREE_AT_X = "the free set is taken at x in place of the Cauchy point"
PINNED_DRIFT = "pinned coordinates are overwritten by the drift"
EVICT_NEWEST = "the newest pair is evicted"
STORE_ANYWAY = "a pair with s^T y <= 1e-7 y^T y is stored anyway"
BUGS = (OUT_OF_ORDER, NO_CROSS_TERM, C_NOT_ADVANCED, W_WITHOUT_THETA, THETA_OLDEST, PAPER_SIGN, ALPHA_NO_LOWER, FREE_AT_X,
        PINNED_DRIFT, EVICT_NEWEST, STORE_ANYWAY)


class History:
    """the ring and theta; `bug` one of EVICT_NEWEST, THETA_OLDEST, STORE_ANYWAY or None"""

    def __init__(self, m, bug=None):
        self.m, self.bug, self.S, self.Y, self.theta = m, bug, [], [], 1.0

    def update(self, s, y):
        dot = step_lib.tree_dot
        sy, yy = dot(s, y), dot(y, y)
        if sy > 1e-7 * yy or (self.bug == STORE_ANYWAY and yy > 0 and sy != 0):
            if len(self.S) == self.m:
                drop = self.m - 1 if self.bug == EVICT_NEWEST else 0
                self.S.pop(drop)
                self.Y.pop(drop)
            self.S.append(s)
            self.Y.append(y)
            S, Y = self.S, self.Y
            self.theta = dot(Y[0], Y[0]) / dot(Y[0], S[0]) if self.bug == THETA_OLDEST else yy / sy


def target(x, g, lo, hi, history, bug=None):
    """algorithm CP and the direct primal method: (x + d, whether a search along d follows)"""
    dot = step_lib.tree_dot
    S, Y, theta = history.S, history.Y, history.theta
    n, p = x.size, len(S)
    if p:
        Sm, Ym = np.array(S).T, np.array(Y).T
        W = np.hstack([Ym, Sm if bug == W_WITHOUT_THETA else theta * Sm])
        A = np.array([[dot(S[i], Y[j]) for j in range(p)] for i in range(p)])
        L = np.tril(A, -1)
        SS = np.array([[dot(S[i], S[j]) for j in range(p)] for i in range(p)])
        MM = np.block([[-np.diag(np.diag(A)), L.T], [L, theta * SS]])
        Mv = lambda v: np.linalg.solve(MM, v)
    else:
        W = np.zeros((n, 0))
        Mv = lambda v: v
    # ---- algorithm CP -----------------------------------------------------------------------------------------------------------
    with np.errstate(divide="ignore", invalid="ignore"):
        tb = np.where(g < 0, (x - hi) / g, np.where(g > 0, (x - lo) / g, np.inf))
    d = np.where(tb > 0, -g, 0.0)
    order = [j for j in np.argsort(tb, kind="stable") if tb[j] > 0]
    if bug == OUT_OF_ORDER and len(order) > 2:
        order = order[:1] + order[:0:-1]
    xc = x.copy()
    pv = W.T @ d
    c = np.zeros(2 * p)
    fp = -dot(d, d)
    fpp = max(1e-12, -theta * fp - pv @ Mv(pv))
    fpp0 = fpp
    dt_min, t_old, i = -fp / fpp, 0.0, 0
    pinned = []
    while i < len(order):
        b = order[i]
        dt = tb[b] - t_old
        if not dt_min >= dt:
            break
        xc[b] = hi[b] if d[b] > 0 else lo[b]
        zb = xc[b] - x[b]
        c = c + dt * pv
        wb = W[b]
        fp = fp + dt * fpp + g[b] * g[b] + theta * g[b] * zb - g[b] * (wb @ Mv(c))
        fpp = fpp - theta * g[b] * g[b] - (0.0 if bug == NO_CROSS_TERM else 2.0 * g[b] * (wb @ Mv(pv))) \
            - g[b] * g[b] * (wb @ Mv(wb))
        fpp = max(1e-12 * fpp0, fpp)
        pv = pv + g[b] * wb
        d[b] = 0.0
        pinned.append(b)
        dt_min = -fp / fpp
        t_old = tb[b]
        i += 1
    dt_min = max(dt_min, 0.0)
    t_old += dt_min
    for j in range(n):
        if j not in pinned or bug == PINNED_DRIFT:
            xc[j] = x[j] + t_old * d[j]
    if bug != C_NOT_ADVANCED:
        c = c + dt_min * pv
    # ---- the direct primal method -------------------------------------------------------------------------------------------------
    at = x if bug == FREE_AT_X else xc
    free = [j for j in range(n) if at[j] != hi[j] and at[j] != lo[j]]
    if not free:
        return xc, False
    WZ = W[free].T
    r = (g + theta * (xc - x) - W @ Mv(c))[free]
    du = -r / theta
    if p:
        v = Mv(WZ @ r)
        N = np.eye(2 * p) - np.column_stack([Mv(col) for col in (WZ @ WZ.T / theta).T])
        v = np.linalg.solve(N, v)
        du = -r / theta + (1.0 if bug == PAPER_SIGN else -1.0) * (WZ.T @ v) / theta ** 2
    alpha = 1.0
    for q, j in enumerate(free):
        if abs(du[q]) < 1e-7:
            continue
        if du[q] > 0:
            alpha = min(alpha, (hi[j] - xc[j]) / du[q])
        elif bug != ALPHA_NO_LOWER:
            alpha = min(alpha, (lo[j] - xc[j]) / du[q])
    out = xc.copy()
    out[free] += alpha * du
    return out, True


def generate(fun, x0, lower, upper, m, limit, gradient_norm=1e-6, bug=None, changes=None):
    """fun(x) -> (f, g) in double.  Returns xs, gs [T + 1, n], fs [T + 1], ended by the projected-gradient test at the
    previous iterate.  `changes`: a list that receives, per iteration, (d with the bug, d without it) from the same iterate
    (the state without the bug is carried alongside): what the bug touches."""
    dot = step_lib.tree_dot
    lo, hi = np.broadcast_to(lower, np.shape(x0)).astype(float), np.broadcast_to(upper, np.shape(x0)).astype(float)
    x = np.clip(np.asarray(x0, dtype=float), lo, hi)
    f, g = fun(x)
    history = History(m, bug)
    clean = History(m) if changes is not None else None
    xs, gs, fs = [x], [g], [f]
    for _ in range(limit + 1):
        goal, search = target(x, g, lo, hi, history, bug)
        if clean is not None:
            changes.append((goal - x, target(x, g, lo, hi, clean)[0] - x))
        if search:
            direction = goal - x
            slope0 = dot(g, direction)
            step, low, high = 1.0, 0.0, None
            for _trial in range(60):
                xn = x + step * direction
                fn, gn = fun(xn)
                slope = dot(gn, direction)
                if not fn <= f + 1e-4 * step * slope0:
                    high = step
                elif abs(slope) <= 0.9 * abs(slope0):
                    break
                elif slope < 0:
                    low = step
                else:
                    high = step
                step = (low + high) / 2.0 if high is not None else step * 4.0
        else:
            xn = goal
            fn, gn = fun(xn)
        clipped = np.clip(xn, lo, hi)
        if not np.array_equal(clipped, xn):
            xn = clipped
            fn, gn = fun(xn)
        history.update(xn - x, gn - g)
        if clean is not None:
            clean.update(xn - x, gn - g)
        pg = np.where(((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0)), 0.0, g)
        x, f, g = xn, fn, gn
        xs.append(x)
        gs.append(g)
        fs.append(f)
        if np.max(np.abs(pg)) < gradient_norm:
            break
    return np.array(xs), np.array(gs), np.array(fs)

