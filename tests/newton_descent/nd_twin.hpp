// nd_twin.hpp — sequential CPU restatement of NewtonDescent (reference solver/newton_descent.h with
// linesearch/armijo.h's Armijo<F, 2>, under Solver::Minimize and Progress::Update) in two summation orders:
//   kRefOrder     inner products and the objective's sum are ascending chains over n, as the reference computes them
//                 over the Eigen stand-in: bit for bit the reference;
//   kDeviceOrder  they are the pairwise trees over the padded width W of the kernel's segment butterflies
//                 (csrc/newton_descent_kernel.hpp, wave_primitives.hpp seg_sum), every vector carried over the W lanes
//                 with the padding lanes computed as the kernel computes them: bit for bit the device.
// The LU, the solve and the chains v_j = sum_i (k d_i) H(i, j) contain no reduction over lanes and are the same in both
// orders.  The search is bounded as the kernel's is (it also ends when alpha * rho == alpha); the counters tell which
// solves got there, and those are not comparable with the reference, which would not have returned.
// kNdDense (examples/user_objective_dense/dense_quartic.hpp) is the one objective with a dense, possibly asymmetric
// Hessian; `Mutation` plants the transposition bugs a symmetric Hessian hides, so that a test can show the recorded inputs
// tell them apart.
// Built with -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "common.h"

namespace nd_twin {

enum Order { kRefOrder = 0, kDeviceOrder = 1 };
// deliberate bugs (tests only): H(j, i) handed to the LU for H(i, j); the chain of the search walking row j for column j
enum Mutation { kNoMutation = 0, kTransposeBeforeLu = 1, kChainWalksRow = 2 };

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
    if (id == kNdRosenbrock) {
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
    if (id == kNdDiagQuadratic) {
      for (int j = 0; j < n; ++j) {
        term[j] = (params[j] * x[j]) * x[j];
        g[j] = (2.0 * params[j]) * x[j];
      }
      return o.sum(term) + params[n];
    }
    if (id == kNdDense) {
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
    const double t = x[0] * x[0] - 2.0;  // kNdQuartic
    g[0] = (4.0 * x[0]) * t;
    return t * t;
  }
  void hessian(const std::vector<double>& x, std::vector<double>& H) const {
    H.assign(static_cast<size_t>(n) * n, 0.0);
    if (id == kNdQuartic) {
      H[0] = (12.0 * x[0]) * x[0] - 8.0;
      return;
    }
    if (id == kNdDense) {  // H(i, j) = S(i, j) as given (column major, never symmetrised), the diagonal + (3 kappa) x_i^2
      const double kappa = params[n * n + n];
      for (int t = 0; t < n * n; ++t) H[t] = params[t];
      for (int i = 0; i < n; ++i) H[i * n + i] = params[i * n + i] + (3.0 * kappa) * (x[i] * x[i]);
      return;
    }
    for (int j = 0; j < n; ++j) {
      if (id == kNdRosenbrock) {
        const bool has_a = j + 1 < n, has_b = j > 0;
        const double a = has_a ? ((1200.0 * x[j]) * x[j] - 400.0 * x[j + 1]) + 2.0 : 0.0;
        H[j * n + j] = (has_a && has_b) ? (a + 200.0) : (has_a ? a : (has_b ? 200.0 : 0.0));
        if (has_a) H[(j + 1) * n + j] = H[j * n + j + 1] = -400.0 * x[j];
      } else {
        H[j * n + j] = 2.0 * params[j];
      }
    }
  }
};

// what the pivot searches of an LU met (the golden generators' assertions)
struct LuStats {
  uint32_t distance[kNdMaxN];  // histogram of p - k over the columns
  uint32_t ties;               // columns whose non-zero maximum was attained more than once (the first one is taken)
  uint32_t zero_columns;       // columns with best == 0: no interchange, no division
};

// PartialPivLU in the pinned order (oracle/eigen_shim/Eigen/LU, csrc/lu_device.hpp); returns the row interchanges made
inline uint32_t lu_factor(std::vector<double>& A, std::vector<int>& piv, int n, LuStats* stats = nullptr) {
  uint32_t interchanges = 0;
  piv.assign(n, 0);
  for (int k = 0; k < n; ++k) {
    int p = k;
    double best = std::fabs(A[k * n + k]);
    for (int i = k + 1; i < n; ++i)
      if (std::fabs(A[k * n + i]) > best) best = std::fabs(A[k * n + i]), p = i;
    piv[k] = p;
    if (stats != nullptr) {
      int attained = 0;
      for (int i = k; i < n; ++i) attained += std::fabs(A[k * n + i]) == best;
      if (best != 0.0 && attained > 1) ++stats->ties;
      if (best == 0.0) ++stats->zero_columns;
      if (p - k < kNdMaxN) ++stats->distance[p - k];
    }
    if (best != 0.0) {
      if (p != k) {
        ++interchanges;
        for (int j = 0; j < n; ++j) std::swap(A[j * n + k], A[j * n + p]);
      }
      for (int i = k + 1; i < n; ++i) A[k * n + i] = A[k * n + i] / A[k * n + k];
    }
    for (int j = k + 1; j < n; ++j)
      for (int i = k + 1; i < n; ++i) A[j * n + i] = A[j * n + i] - A[k * n + i] * A[j * n + k];
  }
  return interchanges;
}
inline void lu_solve(const std::vector<double>& A, const std::vector<int>& piv, double* x, int n) {
  for (int k = 0; k < n; ++k) std::swap(x[k], x[piv[k]]);
  for (int j = 0; j < n; ++j)
    for (int i = j + 1; i < n; ++i) x[i] = x[i] - x[j] * A[j * n + i];
  for (int j = n - 1; j >= 0; --j) {
    x[j] = x[j] / A[j * n + j];
    for (int i = 0; i < j; ++i) x[i] = x[i] - x[j] * A[j * n + i];
  }
}

// ||H||_F ||H^-1||_F through the same LU (the stopping decision only; see csrc/hessian_condition_device.hpp)
inline double condition(std::vector<double> A, int n) {
  double sh = 0.0;
  for (double v : A) sh += v * v;
  std::vector<int> piv;
  lu_factor(A, piv, n);
  double si = 0.0;
  std::vector<double> cb(n);
  for (int c = 0; c < n; ++c) {
    for (int i = 0; i < n; ++i) cb[i] = (i == c) ? 1.0 : 0.0;
    lu_solve(A, piv, cb.data(), n);
    for (int i = 0; i < n; ++i) si += cb[i] * cb[i];
  }
  return std::sqrt(sh) * std::sqrt(si);
}

struct SearchResult {
  double alpha, f;
  uint32_t trials;
  bool fixed_point;
};

// Armijo<F, 2>::Search (armijo.h:82-102) from x along d, given f, g, H at x; leaves the last trial point and its
// gradient in xt, gt
inline SearchResult armijo(const Objective& obj, const Ops& o, const nd_config& c, const std::vector<double>& x, double f,
                           const std::vector<double>& g, const std::vector<double>& H, const std::vector<double>& d,
                           std::vector<double>& xt, std::vector<double>& gt, Mutation mutation = kNoMutation) {
  const int n = obj.n, L = o.L;
  double alpha = 1.0;
  xt.assign(L, 0.0);
  for (int j = 0; j < L; ++j) xt[j] = x[j] + alpha * d[j];
  SearchResult r{alpha, obj.eval(o, xt, gt), 1, false};
  const double gd = o.dot(g, d);
  const double kq = (0.5 * c.armijo_c) * c.armijo_c;
  std::vector<double> kd(L), v(L, 0.0);
  for (int j = 0; j < L; ++j) kd[j] = kq * d[j];
  for (int j = 0; j < n; ++j) {
    double s = kd[0] * (mutation == kChainWalksRow ? H[j] : H[j * n]);
    for (int i = 1; i < n; ++i) s = s + kd[i] * (mutation == kChainWalksRow ? H[i * n + j] : H[j * n + i]);
    v[j] = s;
  }
  const double cache = c.armijo_c * gd + o.dot(v, d);
  while (r.f > f + alpha * cache) {
    if (alpha * c.armijo_rho == alpha) {
      r.fixed_point = true;
      break;
    }
    alpha = alpha * c.armijo_rho;
    for (int j = 0; j < L; ++j) xt[j] = x[j] + alpha * d[j];
    r.f = obj.eval(o, xt, gt);
    ++r.trials;
  }
  r.alpha = alpha;
  return r;
}

enum { kContinue = 0, kIterationLimit = 1, kXDelta = 2, kFDelta = 3, kGradient = 4, kCondition = 5 };  // progress.h

// trajectory (may be null): per Progress::Update one row (num_iterations, status, value, x_delta, f_delta,
// gradient_norm) and the iterate, at most `capacity` of them
struct Trajectory {
  int capacity;
  double* rows;
  double* xs;
  int count;
};

inline void solve_one(const Objective& obj, Order order, int W, const nd_stop& st, double condition_stop,
                      const nd_config& c, const double* x0, double* x_out, double* f_out, double* g_out,
                      nd_progress* prog, nd_counters* counters, Trajectory* traj = nullptr,
                      Mutation mutation = kNoMutation) {
  const int n = obj.n;
  const Ops o{order, n, order == kDeviceOrder ? W : n};
  const int L = o.L;
  std::vector<double> x(L, 0.0), g, gt, xt, H, A, d(L);
  std::vector<int> piv;
  for (int j = 0; j < n; ++j) x[j] = x0[j];
  double f = obj.eval(o, x, g);
  uint32_t nfev = 1, trials_total = 0, it = 0;
  nd_counters cnt{};
  cnt.min_condition_margin = std::numeric_limits<double>::infinity();
  LuStats lus{};
  obj.hessian(x, H);
  int xv = 0, fv = 0, status = kContinue;
  double x_delta = 0, f_delta = 0, gnorm = 0;
  std::vector<double> past(st.past > 0 ? st.past : 1);
  int past_pos = 0;
  bool past_init = false;
  do {
    nfev += 1;  // function(current.x, &gradient, &hessian)
    A.resize(H.size());
    for (size_t t = 0; t < H.size(); ++t) A[t] = H[t] + 0.0;   // + safe_guard * Identity, element by element
    for (int j = 0; j < n; ++j) A[j * n + j] = H[j * n + j] + c.safe_guard;
    if (mutation == kTransposeBeforeLu) {
      const std::vector<double> At = A;
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) A[j * n + i] = At[i * n + j];
    }
    cnt.interchanges += lu_factor(A, piv, n, &lus);
    for (int j = 0; j < L; ++j) d[j] = -g[j];
    lu_solve(A, piv, d.data(), n);
    for (int j = n; j < L; ++j) d[j] = 0.0;
    nfev += 1;  // Armijo's function(x, &gradient, &hessian)
    const double fprev = f;
    const std::vector<double> xprev = x;
    const SearchResult r = armijo(obj, o, c, x, f, g, H, d, xt, gt, mutation);
    nfev += r.trials + 1;  // the trials, and the state rebuild of Solver::Minimize
    trials_total += r.trials;
    cnt.max_trials = std::max(cnt.max_trials, r.trials);
    if (r.fixed_point) ++cnt.fixed_point;
    if (r.alpha == 1.0) ++cnt.alpha_one_steps; else ++cnt.alpha_less_steps;
    x = xt;
    f = r.f;
    g = gt;
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
    if (!decided) {
      obj.hessian(x, H);
      if (condition_stop > 0) {
        const double cond = condition(H, n);
        ++cnt.conditions;
        cnt.min_condition_margin = std::min(cnt.min_condition_margin, std::fabs(cond - condition_stop) / condition_stop);
        if (cond > condition_stop) status = kCondition;
      }
    }
    if (traj != nullptr && traj->count < traj->capacity) {
      double* row = traj->rows + 6 * traj->count;
      row[0] = it; row[1] = status; row[2] = f; row[3] = x_delta; row[4] = f_delta; row[5] = gnorm;
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
  prog->sum_k = trials_total;
  prog->x_delta = x_delta;
  prog->f_delta = f_delta;
  prog->gradient_norm = gnorm;
  cnt.pivot_ties = lus.ties;
  cnt.zero_columns = lus.zero_columns;
  for (int t = 0; t < kNdMaxN; ++t) cnt.pivot_distance[t] = lus.distance[t];
  if (counters) *counters = cnt;
}

}  // namespace nd_twin
