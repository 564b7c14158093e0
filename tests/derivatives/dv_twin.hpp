// dv_twin.hpp — the CPU twin of the derivative-check kernels (cppnumericalsolvers_amd/csrc/derivative_check_kernel.hpp):
// the four routines of the reference's utils/derivatives.h restated operation for operation over oracle::Objective, in
// two summation orders:
//   kRefOrder     the objective's sums are ascending chains over n, as the reference-shaped host functors of
//                 ref_harness.cpp compute them: bit for bit the reference's ComputeFiniteGradient / ComputeFiniteHessian
//                 and the two verdicts;
//   kDeviceOrder  they are the pairwise trees over the zero-padded width W x E of the kernel (the in-lane tree over a
//                 lane's E consecutive coordinates, then the segment butterfly): bit for bit the device.
// Rosenbrock and DiagQuadratic are the ones of oracle/lbfgs_oracle.hpp; the quartic, the dense quartic and the planted
// functor restate examples/user_objective_quartic, examples/user_objective_dense and tests/derivatives/planted.hpp.
// Beyond the reference: the step and tolerance overrides, the worst excess with its index, and the nonfinite count
// (include/mi355_lbfgs.h, mi355_derivative_report).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../oracle/lbfgs_oracle.hpp"
#include "common.h"

namespace dv_twin {

enum Order { kRefOrder = 0, kDeviceOrder = 1 };

// x_j as seg_coordinate hands it to every lane of the segment: exact, a -0.0 arrives as +0.0 (device order only)
inline double coordinate(double v, const oracle::Reducer& red) {
  return red.kind == oracle::Reduction::Butterfly ? v + 0.0 : v;
}
// a sum whose in-lane part is an ascending chain over the lane's `elems` coordinates (examples/user_objective_dense)
inline double chain_then_tree(const double* v, int n, const oracle::Reducer& red, int elems) {
  if (red.kind != oracle::Reduction::Butterfly || elems <= 1) return red.sum(v, n);
  const int groups = red.width / elems;
  std::vector<double> t(static_cast<size_t>(groups));
  for (int l = 0; l < groups; ++l) {
    double acc = 0.0;
    for (int e = 0; e < elems; ++e) {
      const int i = l * elems + e;
      const double term = (i < n) ? v[i] : 0.0;
      acc = (e == 0) ? term : acc + term;
    }
    t[static_cast<size_t>(l)] = acc;
  }
  return red.sum(t.data(), groups, groups);
}

struct DiagQuadraticHess final : oracle::Objective {
  oracle::DiagQuadratic q;
  double eval(const double* x, double* g, int n, const oracle::Reducer& red) const override { return q.eval(x, g, n, red); }
  bool hess_full(const double*, double* H, int n) const override {
    for (int t = 0; t < n * n; ++t) H[t] = 0.0;
    for (int i = 0; i < n; ++i) H[i * n + i] = 2.0 * q.a[static_cast<size_t>(i)];
    return true;
  }
};

// f = (x_0^2 - 2)^2 in n dimensions: t = x x - 2, f = t t, g_0 = (4 x) t, H_00 = (12 x) x - 8
struct Quartic final : oracle::Objective {
  mutable bool device = false;
  double eval(const double* x, double* g, int n, const oracle::Reducer& red) const override {
    const double x0 = coordinate(x[0], red);
    const double t = x0 * x0 - 2.0;
    for (int i = 0; i < n; ++i) g[i] = 0.0;
    g[0] = (4.0 * x0) * t;
    device = red.kind == oracle::Reduction::Butterfly;
    return t * t;
  }
  bool hess_full(const double* x, double* H, int n) const override {
    const double x0 = device ? x[0] + 0.0 : x[0];
    for (int t = 0; t < n * n; ++t) H[t] = 0.0;
    H[0] = (12.0 * x0) * x0 - 8.0;
    return true;
  }
};

// examples/user_objective_dense/dense_quartic.hpp; params: S (column major), b, kappa
struct DenseQuartic final : oracle::Objective {
  const double* params = nullptr;
  int elems = 1;   // coordinates per lane of the device mapping
  double eval(const double* x, double* g, int n, const oracle::Reducer& red) const override {
    const double *S = params, *b = params + n * n, kappa = params[n * n + n];
    std::vector<double> t0(static_cast<size_t>(n)), t1(t0), t2(t0);
    for (int i = 0; i < n; ++i) {
      double s = S[i] * coordinate(x[0], red);
      for (int j = 1; j < n; ++j) s = s + S[j * n + i] * coordinate(x[j], red);
      const double q = x[i] * x[i];
      g[i] = (s - b[i]) + kappa * (q * x[i]);
      t0[static_cast<size_t>(i)] = x[i] * s;
      t1[static_cast<size_t>(i)] = b[i] * x[i];
      t2[static_cast<size_t>(i)] = q * q;
    }
    const double sq = chain_then_tree(t0.data(), n, red, elems), sb = chain_then_tree(t1.data(), n, red, elems),
                 s4 = chain_then_tree(t2.data(), n, red, elems);
    return (0.5 * sq - sb) + (0.25 * kappa) * s4;
  }
  bool hess_full(const double* x, double* H, int n) const override {
    const double *S = params, kappa = params[n * n + n];
    for (int t = 0; t < n * n; ++t) H[t] = S[t];
    for (int i = 0; i < n; ++i) H[i * n + i] = S[i * n + i] + (3.0 * kappa) * (x[i] * x[i]);
    return true;
  }
};

// tests/derivatives/planted.hpp; params: Q (column major, symmetric), c, then kind, i, j, size
struct Planted final : oracle::Objective {
  const double* params = nullptr;
  double eval(const double* x, double* g, int n, const oracle::Reducer& red) const override {
    const double *Q = params, *c = params + n * n, *plant = params + n * n + n;
    const int kind = static_cast<int>(plant[0]), pi = static_cast<int>(plant[1]);
    std::vector<double> term(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
      double s = Q[i] * coordinate(x[0], red);
      for (int j = 1; j < n; ++j) s = s + Q[j * n + i] * coordinate(x[j], red);
      const double q = x[i] * x[i];
      double gi = s + c[i] * (q * x[i]);
      if (kind == 1 && i == pi) gi = gi + plant[3];
      g[i] = gi;
      term[static_cast<size_t>(i)] = 0.5 * (x[i] * s) + (0.25 * c[i]) * (q * q);
    }
    return red.sum(term.data(), n);
  }
  bool hess_full(const double* x, double* H, int n) const override {
    const double *Q = params, *c = params + n * n, *plant = params + n * n + n;
    const int kind = static_cast<int>(plant[0]), pi = static_cast<int>(plant[1]), pj = static_cast<int>(plant[2]);
    for (int t = 0; t < n * n; ++t) H[t] = Q[t];
    for (int i = 0; i < n; ++i) H[i * n + i] = Q[i * n + i] + (3.0 * c[i]) * (x[i] * x[i]);
    if ((kind == 2 || kind == 3) && pi >= 0 && pi < n && pj >= 0 && pj < n) {
      H[pj * n + pi] = H[pj * n + pi] + plant[3];
      if (kind == 2 && pi != pj) H[pi * n + pj] = H[pi * n + pj] + plant[3];
    }
    return true;
  }
};

inline double std_max(double a, double b) { return (a < b) ? b : a; }
inline double step_of(double factor, double xd) { return factor * std_max(std::fabs(xd), 1.0); }
inline double sqrt_eps() { return std::sqrt(std::numeric_limits<double>::epsilon()); }

struct Evaluator {
  const oracle::Objective& obj;
  const oracle::Reducer& red;
  int n;
  mutable std::vector<double> g;
  double operator()(const std::vector<double>& x) const {
    g.resize(static_cast<size_t>(n));
    return obj.eval(x.data(), g.data(), n, red);
  }
};

// utils/derivatives.h:37-83
inline void finite_gradient(const Evaluator& f, const double* x0, int accuracy, double factor, double* grad) {
  static const double coeff[4][8] = {{1, -1}, {1, -8, 8, -1}, {-1, 9, -45, 45, -9, 1}, {3, -32, 168, -672, 672, -168, 32, -3}};
  static const double coeff2[4][8] = {{1, -1}, {-2, -1, 1, 2}, {-3, -2, -1, 1, 2, 3}, {-4, -3, -2, -1, 1, 2, 3, 4}};
  static const double dd[4] = {2, 12, 60, 840};
  const int n = f.n;
  std::vector<double> x(x0, x0 + n);
  const int inner_steps = 2 * (accuracy + 1);
  for (int d = 0; d < n; ++d) {
    const double h = step_of(factor, x0[d]);
    const double dd_val = dd[accuracy] * h;
    double sum = 0.0;
    for (int s = 0; s < inner_steps; ++s) {
      const double tmp = x[static_cast<size_t>(d)];
      x[static_cast<size_t>(d)] = tmp + coeff2[accuracy][s] * h;
      sum = sum + coeff[accuracy][s] * f(x);
      x[static_cast<size_t>(d)] = tmp;
    }
    grad[d] = sum / dd_val;
  }
}

// utils/derivatives.h:86-252; hessian: column major n x n (symmetric by construction)
inline void finite_hessian(const Evaluator& f, const double* x0, int accuracy, double factor, double* hessian) {
  const int n = f.n;
  std::vector<double> x(x0, x0 + n);
  const double f0 = f(x);
  auto at = [&](int i, int j, double ci, double hi, double cj, double hj) {
    x.assign(x0, x0 + n);
    x[static_cast<size_t>(i)] = x0[i] + ci * hi;
    x[static_cast<size_t>(j)] = x0[j] + cj * hj;
    return f(x);
  };
  for (int i = 0; i < n; ++i) {
    const double hi = step_of(factor, x0[i]);
    x.assign(x0, x0 + n);
    x[static_cast<size_t>(i)] = x0[i] + hi;
    const double f_plus = f(x);
    x[static_cast<size_t>(i)] = x0[i] - hi;
    const double f_minus = f(x);
    hessian[i * n + i] = (f_plus - 2 * f0 + f_minus) / (hi * hi);
    for (int j = i + 1; j < n; ++j) {
      const double hj = step_of(factor, x0[j]);
      double v;
      if (accuracy == 0) {
        const double f_pp = at(i, j, 1, hi, 1, hj), f_pm = at(i, j, 1, hi, -1, hj), f_mp = at(i, j, -1, hi, 1, hj),
                     f_mm = at(i, j, -1, hi, -1, hj);
        v = (f_pp - f_pm - f_mp + f_mm) / (4 * hi * hj);
      } else {
        const double h = (hi + hj) / 2;
        double term1 = 0, term2 = 0, term3 = 0, term4 = 0;
        term1 += at(i, j, 1, h, -2, h);
        term1 += at(i, j, 2, h, -1, h);
        term1 += at(i, j, -2, h, 1, h);
        term1 += at(i, j, -1, h, 2, h);
        term2 += at(i, j, -1, h, -2, h);
        term2 += at(i, j, -2, h, -1, h);
        term2 += at(i, j, 1, h, 2, h);
        term2 += at(i, j, 2, h, 1, h);
        term3 += at(i, j, 2, h, -2, h);
        term3 += at(i, j, -2, h, 2, h);
        term3 -= at(i, j, -2, h, -2, h);
        term3 -= at(i, j, 2, h, 2, h);
        term4 += at(i, j, -1, h, -1, h);
        term4 += at(i, j, 1, h, 1, h);
        term4 -= at(i, j, 1, h, -1, h);
        term4 -= at(i, j, -1, h, 1, h);
        v = (-63 * term1 + 63 * term2 + 44 * term3 + 74 * term4) / (600 * h * h);
      }
      hessian[j * n + i] = v;
      hessian[i * n + j] = v;
    }
  }
}

// :271-278, :299-309 over `count` entries; adds to *nonfinite
inline void compare(const double* actual, const double* expected, int count, double tol, int32_t* ok, int32_t* worst_index,
                    double* worst_excess, int32_t* nonfinite) {
  double worst = -1.0;
  int index = -1;
  bool failed = false;
  const double inf = std::numeric_limits<double>::infinity();
  for (int t = 0; t < count; ++t) {
    const double aa = std::fabs(actual[t]), ae = std::fabs(expected[t]);
    const double scale = std_max(std_max(aa, ae), 1.0);
    const double diff = std::fabs(actual[t] - expected[t]);
    const double bound = tol * scale;
    if (diff > bound) failed = true;
    if (!(aa < inf) || !(ae < inf)) ++*nonfinite;
    const double excess = diff / bound;
    if (excess > worst) {
      worst = excess;
      index = t;
    }
  }
  *ok = failed ? 0 : 1;
  *worst_index = index;
  *worst_excess = index < 0 ? 0.0 : worst;
}

// everything the entry point returns for one point; hess / hess_fd null: gradient only
inline void check_one(const oracle::Objective& obj, int n, Order order, int width, const dv_config& c, const double* x,
                      double* f, double* grad, double* grad_fd, double* hess, double* hess_fd, dv_report* report) {
  oracle::Reducer red;
  red.kind = (order == kDeviceOrder) ? oracle::Reduction::Butterfly : oracle::Reduction::Sequential;
  red.width = width;
  const Evaluator ev{obj, red, n, {}};
  *f = obj.eval(x, grad, n, red);
  finite_gradient(ev, x, c.gradient_accuracy, c.gradient_step > 0.0 ? c.gradient_step : sqrt_eps(), grad_fd);
  dv_report r;
  r.gradient_ok = r.hessian_ok = -1;
  r.gradient_worst_index = r.hessian_worst_index = -1;
  r.nonfinite = r.pad = 0;
  r.gradient_worst_excess = r.hessian_worst_excess = 0.0;
  compare(grad, grad_fd, n, c.gradient_tolerance > 0.0 ? c.gradient_tolerance : static_cast<double>(1e-2f),
          &r.gradient_ok, &r.gradient_worst_index, &r.gradient_worst_excess, &r.nonfinite);
  if (hess != nullptr && hess_fd != nullptr) {
    finite_hessian(ev, x, c.hessian_accuracy, c.hessian_step > 0.0 ? c.hessian_step : sqrt_eps(), hess_fd);
    if (obj.hess_full(x, hess, n))
      compare(hess, hess_fd, n * n, c.hessian_tolerance > 0.0 ? c.hessian_tolerance : static_cast<double>(1e-1f),
              &r.hessian_ok, &r.hessian_worst_index, &r.hessian_worst_excess, &r.nonfinite);
  }
  *report = r;
}

}  // namespace dv_twin
