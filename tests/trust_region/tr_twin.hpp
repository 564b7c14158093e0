// tr_twin.hpp — sequential CPU restatement of TrustRegionNewton (reference solver/trust_region_newton.h under
// Solver::Minimize and Progress::Update) in two summation orders:
//   kRefOrder     inner products and the objective's sum are ascending chains over n, as the reference computes them
//                 over the Eigen stand-in: bit for bit the reference;
//   kDeviceOrder  they are the pairwise trees over the padded width W of the kernel's segment butterflies
//                 (csrc/trust_region_kernel.hpp, wave_primitives.hpp seg_sum), every vector carried over the W lanes with
//                 the padding lanes computed as the kernel computes them: bit for bit the device.
// H d is the ascending row sum in both (the kernel forms it that way).  kTrDense
// (examples/user_objective_dense/dense_quartic.hpp) is the one objective with a dense, possibly asymmetric Hessian;
// `Mutation` plants the transposed product a symmetric Hessian hides.  Built with -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "common.h"

namespace tr_twin {

enum Order { kRefOrder = 0, kDeviceOrder = 1 };
// a deliberate bug (tests only): H d walking column j of H for row j
enum Mutation { kNoMutation = 0, kProductWalksColumn = 1 };

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
  double dot(const std::vector<double>& a, const std::vector<double>& b) const {
    std::vector<double> t(L);
    for (int i = 0; i < L; ++i) t[i] = a[i] * b[i];
    return sum(t);
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

// the objectives, with the device functors' formulas (csrc/objectives.hpp); vectors of length L, H n x n column major
struct Objective {
  int id, n;
  const double* params;
  double eval(const Ops& o, const std::vector<double>& x, std::vector<double>& g) const {
    const int L = o.L;
    std::vector<double> term(L, 0.0);
    g.assign(L, 0.0);
    if (id == kTrRosenbrock) {
      for (int j = 0; j < L; ++j) {
        const bool has_a = j + 1 < n, has_b = j > 0 && j < n;
        const double xn = (j + 1 < L) ? x[j + 1] : 0.0;
        const double t1 = 1.0 - x[j];
        const double t2 = xn - x[j] * x[j];
        if (has_a) term[j] = t1 * t1 + (100.0 * t2) * t2;
        const double a = -2.0 * (1.0 - x[j]) + (200.0 * t2) * (-2.0 * x[j]);
        const double b = has_b ? 200.0 * (x[j] - x[j - 1] * x[j - 1]) : 0.0;
        g[j] = (has_a && has_b) ? (a + b) : (has_a ? a : (has_b ? b : 0.0));
      }
      return o.sum(term);
    }
    if (id == kTrDiagQuadratic) {
      for (int j = 0; j < n; ++j) {
        term[j] = (params[j] * x[j]) * x[j];
        g[j] = (2.0 * params[j]) * x[j];
      }
      return o.sum(term) + params[n];
    }
    if (id == kTrDense) {
      // S x row by row, ascending in j with the first term a product; x_j reaches the other lanes of the device through a
      // butterfly over zeros (seg_coordinate): x_j + 0.0
      const double *S = params, *b = params + n * n, kappa = params[n * n + n];
      std::vector<double> lin(L, 0.0), quart(L, 0.0);
      for (int i = 0; i < n; ++i) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) {
          const double xj = (o.order == kDeviceOrder) ? x[j] + 0.0 : x[j];
          s = (j == 0) ? S[i] * xj : s + S[j * n + i] * xj;
        }
        const double q = x[i] * x[i];
        g[i] = (s - b[i]) + kappa * (q * x[i]);
        term[i] = x[i] * s;
        lin[i] = b[i] * x[i];
        quart[i] = q * q;
      }
      return (0.5 * o.sum(term) - o.sum(lin)) + (0.25 * kappa) * o.sum(quart);
    }
    const double t = x[0] * x[0] - 2.0;  // kTrQuartic
    g[0] = (4.0 * x[0]) * t;
    return t * t;
  }
  void hessian(const std::vector<double>& x, std::vector<double>& H) const {
    H.assign(static_cast<size_t>(n) * n, 0.0);
    if (id == kTrDense) {  // H(i, j) = S(i, j) as given (column major, never symmetrised), the diagonal + (3 kappa) x_i^2
      const double kappa = params[n * n + n];
      for (int t = 0; t < n * n; ++t) H[t] = params[t];
      for (int i = 0; i < n; ++i) H[i * n + i] = params[i * n + i] + (3.0 * kappa) * (x[i] * x[i]);
      return;
    }
    for (int j = 0; j < n; ++j) {
      if (id == kTrRosenbrock) {
        const bool has_a = j + 1 < n, has_b = j > 0;
        const double a = has_a ? ((1200.0 * x[j]) * x[j] - 400.0 * x[j + 1]) + 2.0 : 0.0;
        H[j * n + j] = (has_a && has_b) ? (a + 200.0) : (has_a ? a : (has_b ? 200.0 : 0.0));
        if (has_a) H[(j + 1) * n + j] = H[j * n + j + 1] = -400.0 * x[j];
      } else if (id == kTrDiagQuadratic) {
        H[j * n + j] = 2.0 * params[j];
      } else {
        H[0] = (12.0 * x[0]) * x[0] - 8.0;
      }
    }
  }
};

// ||H||_F ||H^-1||_F through LU with partial pivoting (the stopping decision only; see hessian_condition_device.hpp)
inline double condition(std::vector<double> A, int n) {
  double sh = 0.0;
  for (double v : A) sh += v * v;
  std::vector<int> piv(n);
  for (int k = 0; k < n; ++k) {
    int p = k;
    double best = std::fabs(A[k * n + k]);
    for (int i = k + 1; i < n; ++i)
      if (std::fabs(A[k * n + i]) > best) best = std::fabs(A[k * n + i]), p = i;
    piv[k] = p;
    if (best != 0.0) {
      if (p != k)
        for (int j = 0; j < n; ++j) std::swap(A[j * n + k], A[j * n + p]);
      for (int i = k + 1; i < n; ++i) A[k * n + i] = A[k * n + i] / A[k * n + k];
    }
    for (int j = k + 1; j < n; ++j)
      for (int i = k + 1; i < n; ++i) A[j * n + i] = A[j * n + i] - A[k * n + i] * A[j * n + k];
  }
  double si = 0.0;
  std::vector<double> cb(n);
  for (int c = 0; c < n; ++c) {
    for (int i = 0; i < n; ++i) cb[i] = (i == c) ? 1.0 : 0.0;
    for (int k = 0; k < n; ++k) std::swap(cb[k], cb[piv[k]]);
    for (int j = 0; j < n; ++j)
      for (int i = j + 1; i < n; ++i) cb[i] = cb[i] - cb[j] * A[j * n + i];
    for (int j = n - 1; j >= 0; --j) {
      cb[j] = cb[j] / A[j * n + j];
      for (int i = 0; i < j; ++i) cb[i] = cb[i] - cb[j] * A[j * n + i];
    }
    for (int i = 0; i < n; ++i) si += cb[i] * cb[i];
  }
  return std::sqrt(sh) * std::sqrt(si);
}

enum { kContinue = 0, kIterationLimit = 1, kXDelta = 2, kFDelta = 3, kGradient = 4, kCondition = 5 };  // progress.h

inline void solve_one(const Objective& obj, Order order, int W, const tr_stop& st, double condition_stop,
                      const tr_config& c, const double* x0, double* x_out, double* f_out, double* g_out,
                      tr_progress* prog, tr_counters* counters = nullptr, Mutation mutation = kNoMutation) {
  const int n = obj.n;
  tr_counters cnt{};
  cnt.min_condition_margin = std::numeric_limits<double>::infinity();
  const Ops o{order, n, order == kDeviceOrder ? W : n};
  const int L = o.L;
  std::vector<double> x(L, 0.0), g, gt, xt(L), H;
  for (int j = 0; j < n; ++j) x[j] = x0[j];
  auto hess_times = [&](const std::vector<double>& d) {
    std::vector<double> out(L, 0.0);
    for (int j = 0; j < n; ++j) {
      double s = (mutation == kProductWalksColumn ? H[j * n] : H[j]) * d[0];
      for (int k = 1; k < n; ++k) s = s + (mutation == kProductWalksColumn ? H[j * n + k] : H[j + k * n]) * d[k];
      out[j] = s;
    }
    return out;
  };
  double f = obj.eval(o, x, g);
  uint32_t nfev = 1, cg_total = 0, it = 0;
  double radius = c.initial_radius;
  obj.hessian(x, H);
  const int retry_limit = std::min(std::max(c.rejection_retry_limit, 0), 1000);
  const int cg_max = std::max(c.cg_max_iterations_floor, 0);  // the reference's dim_ is 0 here (InitializeSolver)
  int xv = 0, fv = 0, status = kContinue;
  double x_delta = 0, f_delta = 0, gnorm = 0;
  std::vector<double> past(st.past > 0 ? st.past : 1);
  int past_pos = 0;
  bool past_init = false;
  do {
    nfev += 1;  // function(current.x, &gradient, &hessian)
    const double gi = o.amax(g);
    const double forcing = std::min(0.5, std::sqrt(gi));
    const double tol = c.cg_forcing_coefficient * forcing * gi;
    const double fprev = f;
    const std::vector<double> xprev = x;
    for (int retry = 0; retry < retry_limit; ++retry) {
      std::vector<double> p(L, 0.0), r = g, d(L);
      for (int j = 0; j < L; ++j) d[j] = -g[j];
      double rr = o.dot(r, r);
      bool hit = false;
      uint32_t cgi = 0;
      auto to_boundary = [&]() {
        const double a = o.dot(d, d);
        const double b = 2.0 * o.dot(p, d);
        const double cc = o.dot(p, p) - radius * radius;
        const double disc = b * b - 4.0 * a * cc;
        const double tau = (-b + std::sqrt(std::max(disc, 0.0))) / (2.0 * a);
        for (int j = 0; j < L; ++j) p[j] = p[j] + tau * d[j];
        hit = true;
        ++cnt.boundary_hits;
      };
      if (!(std::sqrt(rr) <= tol)) {
        for (int k = 0; k < cg_max; ++k) {
          ++cgi;
          const std::vector<double> hd = hess_times(d);
          const double curv = o.dot(d, hd);
          if (!(curv > 0.0)) { ++cnt.negative_curvature_exits; to_boundary(); break; }
          const double alpha = rr / curv;
          std::vector<double> pc(L);
          for (int j = 0; j < L; ++j) pc[j] = p[j] + alpha * d[j];
          if (std::sqrt(o.dot(pc, pc)) >= radius) { to_boundary(); break; }
          p = pc;
          for (int j = 0; j < L; ++j) r[j] = r[j] + alpha * hd[j];
          const double rr_new = o.dot(r, r);
          if (std::sqrt(rr_new) <= tol) break;
          const double beta = rr_new / rr;
          for (int j = 0; j < L; ++j) d[j] = -r[j] + beta * d[j];
          rr = rr_new;
        }
      }
      for (int j = n; j < L; ++j) p[j] = 0.0;
      for (int j = 0; j < L; ++j) xt[j] = x[j] + p[j];
      const double ft = obj.eval(o, xt, gt);
      nfev += 1;
      const double predicted = -o.dot(g, p) - 0.5 * o.dot(p, hess_times(p));
      const double actual = fprev - ft;
      const double rho = (predicted <= 0.0) ? -std::numeric_limits<double>::infinity() : actual / predicted;
      const double radius_before = radius;
      if (rho < c.rho_low) radius *= c.shrink_factor;
      else if (rho > c.rho_high && hit) radius = std::min(c.expand_factor * radius, c.max_radius);
      cg_total += cgi;
      cnt.max_cg_iterations = std::max(cnt.max_cg_iterations, cgi);
      if (cgi >= 3) ++cnt.subproblems_of_3_cg_iterations;
      if (rho > c.acceptance_threshold) {
        x = xt; f = ft; g = gt; nfev += 1;
        obj.hessian(x, H);
        break;
      }
      if (radius <= c.min_radius) break;
      if (radius == radius_before) {  // the remaining retries repeat this one exactly
        const uint32_t left = static_cast<uint32_t>(retry_limit - retry - 1);
        nfev += left;
        cg_total += left * cgi;
        break;
      }
    }
    // Progress::Update
    ++it;
    f_delta = std::fabs(f - fprev);
    std::vector<double> dx(L);
    for (int j = 0; j < L; ++j) dx[j] = x[j] - xprev[j];
    x_delta = o.amax(dx);
    gnorm = o.amax(g);
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
        if (++fv >= st.f_delta_violations) { status = kFDelta; decided = true; }
      } else fv = 0;
    }
    if (!decided && st.past > 0) {
      if (!past_init) { for (auto& v : past) v = f; past_init = true; past_pos = 0; }
      if (static_cast<int>(it) > st.past) {
        if (std::fabs(past[past_pos] - f) / std::max(1.0, std::fabs(f)) < st.past_delta) { status = kFDelta; decided = true; }
      }
      if (!decided) { past[past_pos] = f; past_pos = (past_pos + 1 == st.past) ? 0 : past_pos + 1; }
    }
    if (!decided && st.gradient_norm > 0) {
      const double scale = st.gradient_norm_relative ? std::max(1.0, o.amax(x)) : 1.0;
      if (gnorm < st.gradient_norm * scale) { status = kGradient; decided = true; }
    }
    if (!decided && condition_stop > 0) {
      const double cond = condition(H, n);
      ++cnt.conditions;
      cnt.min_condition_margin = std::min(cnt.min_condition_margin, std::fabs(cond - condition_stop) / condition_stop);
      if (cond > condition_stop) status = kCondition;
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
  prog->sum_k = cg_total;
  prog->x_delta = x_delta;
  prog->f_delta = f_delta;
  prog->gradient_norm = gnorm;
  if (counters) *counters = cnt;
}

}  // namespace tr_twin
