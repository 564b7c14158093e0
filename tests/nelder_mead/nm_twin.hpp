// nm_twin.hpp — sequential CPU restatement of NelderMead (reference solver/nelder_mead.h under Solver::Minimize and
// Progress::Update) in two summation orders:
//   kRefOrder     the objective's sum is an ascending chain over n, as the reference harness's functors compute it: bit
//                 for bit the reference (on solves whose rankings met no two equal values, see `tied`);
//   kDeviceOrder  it is the pairwise tree over the padded width W of the kernel's segment butterfly
//                 (csrc/nelder_mead_kernel.hpp, wave_primitives.hpp seg_sum), every vector carried over the W lanes:
//                 bit for bit the device.
// Everything else — simplex, ordering, centroid, moves, stop tests — is element-wise and identical in both.  As the
// kernel, the twin keeps the values of unmoved vertices and counts in nfev what the reference calls.
// Built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "common.h"

namespace nm_twin {

enum Order { kRefOrder = 0, kDeviceOrder = 1 };

inline double tree_sum(const double* v, int len) {  // pairwise tree over a power-of-two length
  if (len == 1) return v[0];
  std::vector<double> h(len / 2);
  for (int i = 0; i < len / 2; ++i) h[i] = v[2 * i] + v[2 * i + 1];
  return tree_sum(h.data(), len / 2);
}

struct Ops {
  Order order;
  int n, L;  // L: vector length carried (n, or the padded width W)
  double sum(const std::vector<double>& t) const {
    if (order == kDeviceOrder) return tree_sum(t.data(), L);
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = (i == 0) ? t[0] : s + t[i];
    return s;
  }
  double amax(const std::vector<double>& a) const {  // lpNorm<Infinity>
    double m = 0.0;
    for (int i = 0; i < L; ++i) {
      const double t = std::fabs(a[i]);
      if (m < t) m = t;
    }
    return m;
  }
};

// the objectives, with the device functors' formulas (csrc/objectives.hpp, examples/user_objective_l1); vectors of length L
struct Objective {
  int id, n;
  const double* params;
  double eval(const Ops& o, const std::vector<double>& x, std::vector<double>* g) const {
    const int L = o.L;
    std::vector<double> term(L, 0.0);
    if (g) g->assign(L, 0.0);
    if (id == kNmRosenbrock) {
      for (int j = 0; j < L; ++j) {
        const bool has_a = j + 1 < n, has_b = j > 0 && j < n;
        const double xn = (j + 1 < L) ? x[j + 1] : 0.0;
        const double t1 = 1.0 - x[j];
        const double t2 = xn - x[j] * x[j];
        if (has_a) term[j] = t1 * t1 + (100.0 * t2) * t2;
        if (g) {
          const double a = -2.0 * (1.0 - x[j]) + (200.0 * t2) * (-2.0 * x[j]);
          const double b = has_b ? 200.0 * (x[j] - x[j - 1] * x[j - 1]) : 0.0;
          (*g)[j] = (has_a && has_b) ? (a + b) : (has_a ? a : (has_b ? b : 0.0));
        }
      }
      return o.sum(term);
    }
    if (id == kNmDiagQuadratic) {
      for (int j = 0; j < n; ++j) {
        term[j] = (params[j] * x[j]) * x[j];
        if (g) (*g)[j] = (2.0 * params[j]) * x[j];
      }
      return o.sum(term) + params[n];
    }
    for (int j = 0; j < n; ++j) {  // kNmL1Quadratic (value only)
      const double d = x[j] - params[j];
      term[j] = std::fabs(d) + (0.5 * d) * d;
    }
    return o.sum(term);
  }
};

enum { kContinue = 0, kIterationLimit = 1, kXDelta = 2, kFDelta = 3, kGradient = 4 };  // progress.h

// *tied: whether any ranking of the solve met two values of which neither is below the other (equal, or a NaN): the
// reference's std::sort places those as its implementation happens to, the project by the lower vertex index
inline void solve_one(const Objective& obj, Order order, int W, const nm_stop& st, const nm_config& c, const double* x0,
                      double* x_out, double* f_out, double* g_out, nm_progress* prog, int32_t* tied,
                      nm_trajectory* traj) {
  const int n = obj.n, nv = n + 1;
  const Ops o{order, n, order == kDeviceOrder ? W : n};
  const int L = o.L;
  const bool first = c.mode != 0;
  std::vector<double> x(L, 0.0), g(L, 0.0), S(static_cast<size_t>(n) * nv), fv(nv), pt(L, 0.0);
  std::vector<int> idx(nv);
  for (int j = 0; j < n; ++j) x[j] = x0[j];
  *tied = 0;
  auto value_at = [&](const std::vector<double>& p) { return obj.eval(o, p, nullptr); };
  auto evaluate_vertex = [&](int v) {
    for (int j = 0; j < n; ++j) pt[j] = S[j + v * n];
    fv[v] = value_at(pt);
  };
  auto make_simplex = [&](const std::vector<double>& p) {  // :202-217
    for (int cidx = 0; cidx < nv; ++cidx)
      for (int r = 0; r < n; ++r) {
        const double ax = std::fabs(p[r]);
        const double delta = (ax > 1e-6) ? 0.05 * ax : 0.001;
        S[r + cidx * n] = (r == cidx - 1) ? p[r] + delta : p[r];
      }
    for (int v = 0; v < nv; ++v) evaluate_vertex(v);
  };
  auto rank_vertices = [&]() {
    for (int v = 0; v < nv; ++v) {
      const bool v_nan = fv[v] != fv[v];
      int r = 0;
      for (int u = 0; u < nv; ++u) {
        const bool u_nan = fv[u] != fv[u];
        const bool u_less = (fv[u] < fv[v]) || (v_nan && !u_nan);
        const bool v_less = (fv[v] < fv[u]) || (u_nan && !v_nan);
        if (u != v && !(fv[u] < fv[v]) && !(fv[v] < fv[u])) *tied = 1;
        r += (u_less || (!v_less && u < v)) ? 1 : 0;
      }
      idx[r] = v;
    }
  };
  double f = first ? obj.eval(o, x, &g) : value_at(x);
  uint32_t nfev = 1, it = 0;
  make_simplex(x);
  int xv = 0, fvio = 0, status = kContinue;
  double x_delta = 0, f_delta = 0, gnorm = 0;
  std::vector<double> past(st.past > 0 ? st.past : 1);
  int past_pos = 0;
  bool past_init = false;
  std::vector<double> xbar(L), xw(L), xr(L), xt(L), d1(L), d2(L), far(L);
  do {
    const double fprev = f;
    const std::vector<double> xprev = x;
    nfev += nv;
    rank_vertices();
    int best = idx[0];
    far.assign(L, 0.0);
    for (int j = 0; j < n; ++j)
      for (int i = 1; i < nv; ++i) {
        const double d = std::fabs(S[j + idx[i] * n] - S[j + best * n]);
        far[j] = (far[j] < d) ? d : far[j];
      }
    if (o.amax(far) < c.degenerate_tol) {
      std::vector<double> xb(L, 0.0);
      for (int j = 0; j < n; ++j) xb[j] = S[j + best * n];
      make_simplex(xb);
      nfev += nv;
      rank_vertices();
      best = idx[0];
    }
    const int worst = idx[n];
    const double f_best = fv[best], f_second = fv[idx[n - 1]], f_worst = fv[worst];
    xbar.assign(L, 0.0);
    xw.assign(L, 0.0);
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int i = 0; i < n; ++i) s = s + S[j + idx[i] * n];
      xbar[j] = s / static_cast<double>(n);
      xw[j] = S[j + worst * n];
    }
    for (int j = 0; j < L; ++j) {
      xr[j] = (1.0 + c.rho) * xbar[j] - c.rho * xw[j];
      d1[j] = xr[j] - xbar[j];
      d2[j] = xr[j] - xw[j];
    }
    bool shrink = (o.amax(d1) < c.degenerate_tol) || (o.amax(d2) < c.degenerate_tol);
    if (!shrink) {
      std::vector<double> xnew = xr;
      const double f_r = value_at(xr);
      nfev += 1;
      double fnew = f_r;
      auto trial = [&](double ca, double cb) {  // ca * xbar + cb * xw, with the sign of cb in the operation
        for (int j = 0; j < L; ++j) xt[j] = ca * xbar[j] + cb * xw[j];
        nfev += 1;
        return value_at(xt);
      };
      if (f_r < f_best) {
        for (int j = 0; j < L; ++j) xt[j] = (1.0 + c.rho * c.xi) * xbar[j] - (c.rho * c.xi) * xw[j];
        nfev += 1;
        const double f_e = value_at(xt);
        if (f_e < f_r) { xnew = xt; fnew = f_e; }
      } else if (f_r < f_second) {
      } else if (f_r < f_worst) {
        for (int j = 0; j < L; ++j) xt[j] = (1.0 + c.rho * c.gamma) * xbar[j] - (c.rho * c.gamma) * xw[j];
        nfev += 1;
        const double f_c = value_at(xt);
        if (f_c <= f_r) { xnew = xt; fnew = f_c; } else shrink = true;
      } else {
        const double f_c = trial(1.0 - c.gamma, c.gamma);
        if (f_c < f_worst) { xnew = xt; fnew = f_c; } else shrink = true;
      }
      if (!shrink) {
        for (int j = 0; j < n; ++j) S[j + worst * n] = xnew[j];
        fv[worst] = fnew;
      }
    }
    if (shrink) {
      nfev += nv;
      for (int i = 1; i < nv; ++i) {
        const int v = idx[i];
        for (int j = 0; j < n; ++j) S[j + v * n] = c.sigma * S[j + v * n] + (1.0 - c.sigma) * S[j + best * n];
        evaluate_vertex(v);
      }
    }
    for (int j = 0; j < n; ++j) x[j] = S[j + best * n];
    nfev += 1;
    f = first ? obj.eval(o, x, &g) : f_best;
    // Progress::Update
    ++it;
    f_delta = std::fabs(f - fprev);
    std::vector<double> dx(L);
    for (int j = 0; j < L; ++j) dx[j] = x[j] - xprev[j];
    x_delta = o.amax(dx);
    if (first) gnorm = o.amax(g);
    status = kContinue;
    bool decided = false;
    if (st.num_iterations > 0 && it > st.num_iterations) { status = kIterationLimit; decided = true; }
    if (!decided) {
      if (st.x_delta > 0 && x_delta < st.x_delta) {
        if (++xv >= st.x_delta_violations) { status = kXDelta; decided = true; }
      } else xv = 0;
    }
    if (!decided) {
      const double fs = st.f_delta_relative ? std::max(std::max(std::fabs(f), std::fabs(fprev)), 1.0) : 1.0;
      if (st.f_delta > 0 && f_delta < st.f_delta * fs) {
        if (++fvio >= st.f_delta_violations) { status = kFDelta; decided = true; }
      } else fvio = 0;
    }
    if (!decided && st.past > 0) {
      if (!past_init) { for (auto& v : past) v = f; past_init = true; past_pos = 0; }
      if (static_cast<int>(it) > st.past) {
        if (std::fabs(past[past_pos] - f) / std::max(1.0, std::fabs(f)) < st.past_delta) { status = kFDelta; decided = true; }
      }
      if (!decided) { past[past_pos] = f; past_pos = (past_pos + 1 == st.past) ? 0 : past_pos + 1; }
    }
    if (!decided && first && st.gradient_norm > 0) {
      const double scale = st.gradient_norm_relative ? std::max(1.0, o.amax(x)) : 1.0;
      if (gnorm < st.gradient_norm * scale) { status = kGradient; decided = true; }
    }
    if (traj != nullptr && traj->count < traj->capacity) {
      double* r = traj->rows + 6 * traj->count;
      r[0] = it; r[1] = status; r[2] = f; r[3] = x_delta; r[4] = f_delta; r[5] = gnorm;
      for (int j = 0; j < n; ++j) traj->xs[traj->count * n + j] = x[j];
      ++traj->count;
    }
  } while (status == kContinue);
  for (int j = 0; j < n; ++j) {
    x_out[j] = x[j];
    g_out[j] = g[j];
  }
  *f_out = f;
  prog->status = status;
  prog->num_iterations = it;
  prog->nfev = nfev;
  prog->sum_k = 0;
  prog->x_delta = x_delta;
  prog->f_delta = f_delta;
  prog->gradient_norm = gnorm;
}

}  // namespace nm_twin
