// ref_harness.cpp — the reference's utils/derivatives.h (UNMODIFIED, from the reference tree) over the Eigen stand-in of
// oracle/eigen_shim, behind a C interface for tests/dv_lib.py.  Compiled at test time (or by
// tests/golden/make_golden_dv.py) into a directory outside the repository; nothing built from it is kept in the tree.
// The functors restate the device functors' formulas (csrc/objectives.hpp, examples/user_objective_quartic,
// examples/user_objective_dense, tests/derivatives/planted.hpp) with sequential sums, so that the twin in reference order
// can match ComputeFiniteGradient, ComputeFiniteHessian and the two verdicts bit for bit.
#include <cmath>
#include <cstdint>

#include "cppoptlib/function.h"
#include "cppoptlib/utils/derivatives.h"
#include "common.h"

namespace {
using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;

class Rosenbrock : public FunctionCRTP<Rosenbrock, double, DifferentiabilityMode::Second> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    const int n = static_cast<int>(x.size());
    double f = 0.0;
    for (int i = 0; i + 1 < n; ++i) {
      const double t1 = 1.0 - x[i];
      const double t2 = x[i + 1] - x[i] * x[i];
      const double term = t1 * t1 + (100.0 * t2) * t2;
      f = (i == 0) ? term : f + term;
    }
    if (gradient) {
      *gradient = VectorType::Zero(n);
      for (int i = 0; i < n; ++i) {
        const bool has_a = (i + 1 < n), has_b = (i > 0);
        double a = 0.0, b = 0.0;
        if (has_a) a = -2.0 * (1.0 - x[i]) + (200.0 * (x[i + 1] - x[i] * x[i])) * (-2.0 * x[i]);
        if (has_b) b = 200.0 * (x[i] - x[i - 1] * x[i - 1]);
        (*gradient)[i] = (has_a && has_b) ? (a + b) : (has_a ? a : b);
      }
    }
    if (hessian) {
      *hessian = MatrixType::Zero(n, n);
      for (int i = 0; i < n; ++i) {
        const bool has_a = (i + 1 < n), has_b = (i > 0);
        const double a = has_a ? ((1200.0 * x[i]) * x[i] - 400.0 * x[i + 1]) + 2.0 : 0.0;
        (*hessian)(i, i) = (has_a && has_b) ? (a + 200.0) : (has_a ? a : (has_b ? 200.0 : 0.0));
        if (has_a) {
          (*hessian)(i, i + 1) = -400.0 * x[i];
          (*hessian)(i + 1, i) = -400.0 * x[i];
        }
      }
    }
    return f;
  }
};

class DiagQuadratic : public FunctionCRTP<DiagQuadratic, double, DifferentiabilityMode::Second> {
 public:
  const double* a = nullptr;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    const int n = static_cast<int>(x.size());
    double f = 0.0;
    if (gradient) *gradient = VectorType::Zero(n);
    for (int i = 0; i < n; ++i) {
      const double term = (a[i] * x[i]) * x[i];
      f = (i == 0) ? term : f + term;
      if (gradient) (*gradient)[i] = (2.0 * a[i]) * x[i];
    }
    if (hessian) {
      *hessian = MatrixType::Zero(n, n);
      for (int i = 0; i < n; ++i) (*hessian)(i, i) = 2.0 * a[i];
    }
    return f + a[n];
  }
};

class Quartic : public FunctionCRTP<Quartic, double, DifferentiabilityMode::Second> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    const int n = static_cast<int>(x.size());
    const double t = x[0] * x[0] - 2.0;
    if (gradient) {
      *gradient = VectorType::Zero(n);
      (*gradient)[0] = (4.0 * x[0]) * t;
    }
    if (hessian) {
      *hessian = MatrixType::Zero(n, n);
      (*hessian)(0, 0) = (12.0 * x[0]) * x[0] - 8.0;
    }
    return t * t;
  }
};

class Dense : public FunctionCRTP<Dense, double, DifferentiabilityMode::Second> {
 public:
  const double* params = nullptr;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    const int n = static_cast<int>(x.size());
    const double *S = params, *b = params + n * n, kappa = params[n * n + n];
    double quad = 0.0, lin = 0.0, quart = 0.0;
    if (gradient) *gradient = VectorType::Zero(n);
    for (int i = 0; i < n; ++i) {
      double s = S[i] * x[0];
      for (int j = 1; j < n; ++j) s = s + S[j * n + i] * x[j];
      const double q = x[i] * x[i];
      if (gradient) (*gradient)[i] = (s - b[i]) + kappa * (q * x[i]);
      const double t0 = x[i] * s, t1 = b[i] * x[i], t2 = q * q;
      quad = (i == 0) ? t0 : quad + t0;
      lin = (i == 0) ? t1 : lin + t1;
      quart = (i == 0) ? t2 : quart + t2;
    }
    if (hessian) {
      *hessian = MatrixType::Zero(n, n);
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) (*hessian)(i, j) = S[j * n + i];
      for (int i = 0; i < n; ++i) (*hessian)(i, i) = S[i * n + i] + (3.0 * kappa) * (x[i] * x[i]);
    }
    return (0.5 * quad - lin) + (0.25 * kappa) * quart;
  }
};

class Planted : public FunctionCRTP<Planted, double, DifferentiabilityMode::Second> {
 public:
  const double* params = nullptr;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    const int n = static_cast<int>(x.size());
    const double *Q = params, *c = params + n * n, *plant = params + n * n + n;
    const int kind = static_cast<int>(plant[0]), pi = static_cast<int>(plant[1]), pj = static_cast<int>(plant[2]);
    double f = 0.0;
    if (gradient) *gradient = VectorType::Zero(n);
    for (int i = 0; i < n; ++i) {
      double s = Q[i] * x[0];
      for (int j = 1; j < n; ++j) s = s + Q[j * n + i] * x[j];
      const double q = x[i] * x[i];
      if (gradient) {
        double gi = s + c[i] * (q * x[i]);
        if (kind == 1 && i == pi) gi = gi + plant[3];
        (*gradient)[i] = gi;
      }
      const double term = 0.5 * (x[i] * s) + (0.25 * c[i]) * (q * q);
      f = (i == 0) ? term : f + term;
    }
    if (hessian) {
      *hessian = MatrixType::Zero(n, n);
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) (*hessian)(i, j) = Q[j * n + i];
      for (int i = 0; i < n; ++i) (*hessian)(i, i) = Q[i * n + i] + (3.0 * c[i]) * (x[i] * x[i]);
      if ((kind == 2 || kind == 3) && pi >= 0 && pi < n && pj >= 0 && pj < n) {
        (*hessian)(pi, pj) = (*hessian)(pi, pj) + plant[3];
        if (kind == 2 && pi != pj) (*hessian)(pj, pi) = (*hessian)(pj, pi) + plant[3];
      }
    }
    return f;
  }
};

template <class F>
void check(const F& fn, int n, int64_t B, int gradient_accuracy, int hessian_accuracy, const double* x0, double* grad_fd,
           double* hess_fd, int32_t* gradient_ok, int32_t* hessian_ok) {
  for (int64_t b = 0; b < B; ++b) {
    typename F::VectorType x(n);
    for (int i = 0; i < n; ++i) x[i] = x0[b * n + i];
    typename F::VectorType g;
    cppoptlib::utils::ComputeFiniteGradient(fn, x, &g, gradient_accuracy);
    for (int i = 0; i < n; ++i) grad_fd[b * n + i] = g[i];
    typename F::MatrixType H;
    cppoptlib::utils::ComputeFiniteHessian(fn, x, &H, hessian_accuracy);
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) hess_fd[(b * n + j) * n + i] = H(i, j);
    gradient_ok[b] = cppoptlib::utils::IsGradientCorrect(fn, x, gradient_accuracy) ? 1 : 0;
    hessian_ok[b] = cppoptlib::utils::IsHessianCorrect(fn, x, hessian_accuracy) ? 1 : 0;
  }
}
}  // namespace

extern "C" int dv_ref_check(int objective, int n, int64_t B, const double* params, int gradient_accuracy,
                            int hessian_accuracy, const double* x0, double* grad_fd, double* hess_fd,
                            int32_t* gradient_ok, int32_t* hessian_ok) {
  if (objective == kDvRosenbrock) {
    Rosenbrock fn;
    check(fn, n, B, gradient_accuracy, hessian_accuracy, x0, grad_fd, hess_fd, gradient_ok, hessian_ok);
  } else if (objective == kDvDiagQuadratic) {
    DiagQuadratic fn;
    fn.a = params;
    check(fn, n, B, gradient_accuracy, hessian_accuracy, x0, grad_fd, hess_fd, gradient_ok, hessian_ok);
  } else if (objective == kDvQuartic) {
    Quartic fn;
    check(fn, n, B, gradient_accuracy, hessian_accuracy, x0, grad_fd, hess_fd, gradient_ok, hessian_ok);
  } else if (objective == kDvDense) {
    Dense fn;
    fn.params = params;
    check(fn, n, B, gradient_accuracy, hessian_accuracy, x0, grad_fd, hess_fd, gradient_ok, hessian_ok);
  } else if (objective == kDvPlanted) {
    Planted fn;
    fn.params = params;
    check(fn, n, B, gradient_accuracy, hessian_accuracy, x0, grad_fd, hess_fd, gradient_ok, hessian_ok);
  } else {
    return -1;
  }
  return 0;
}
