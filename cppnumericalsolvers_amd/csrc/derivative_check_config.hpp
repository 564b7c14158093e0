// derivative_check_config.hpp — kernel arguments of the derivative checker (derivative_check_kernel.hpp), shared by the
// C-ABI (mi355_lbfgs.hip) and the launch templates (derivative_check_launch.hpp).
#pragma once
#include <stdint.h>

#include "../../include/mi355_lbfgs.h"

namespace mi355 {

// sqrt(std::numeric_limits<double>::epsilon()) = sqrt(2^-52), exactly 2^-26: the step factor of utils/derivatives.h
constexpr double kDerivativeSqrtEps = 1.4901161193847656e-08;

// which kernel one call of the dispatch function launches
enum DerivativePhase : int {
  kDerivativeGradient = 0,        // eval -> grad (where grad_out is set), value -> f, the finite-difference gradient
  kDerivativeHessian = 1,         // hess_full -> hess
  kDerivativeFiniteHessian = 2,   // the finite-difference Hessian
};
// what a functor offers beyond its value (registered with its dispatch function)
constexpr int kDerivativeHasEval = 1;
constexpr int kDerivativeHasHessFull = 2;

struct DerivativeArgs {
  const double* x;          // [B][n]
  double* f_out;            // [B] or null
  double* grad_out;         // [B][n] or null
  double* grad_fd_out;      // [B][n] or null
  double* hess_out;         // [B][n][n] or null (column major, as hess_full writes it)
  double* hess_fd_out;      // [B][n][n] or null
  const double* obj_params;
  const double* per_problem;
  int per_problem_stride;
  long long B;
  int n;
  int gradient_accuracy;    // 0..3: the 2, 4, 6, 8 point stencil
  int hessian_accuracy;     // 0: four corners; otherwise the sixteen-point formula
  double gradient_step;     // the factor of max(|x_d|, 1): 2^-26 unless overridden
  double hessian_step;
};

// one launch of the compare kernel: `count` doubles per point on both sides; fills the gradient or the Hessian fields of
// the reports and adds to their nonfinite count
struct DerivativeCompareArgs {
  const double* actual;
  const double* expected;
  mi355_derivative_report* report;   // [B]
  long long B;
  int count;
  double tol;
};

}  // namespace mi355
