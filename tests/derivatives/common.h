// common.h — the C interface shared by the CPU twin of the derivative checker (dv_twin.cpp), the reference harness
// (ref_harness.cpp) and tests/dv_lib.py.  Layouts as include/mi355_lbfgs.h (mi355_derivative_config / _report).
#pragma once
#include <stdint.h>

enum { kDvRosenbrock = 0, kDvDiagQuadratic = 1, kDvQuartic = 100, kDvDense = 101, kDvPlanted = 102 };

struct dv_config {
  int32_t gradient_accuracy, hessian_accuracy;
  double gradient_step, hessian_step, gradient_tolerance, hessian_tolerance;   // 0 = the reference's
};
struct dv_report {
  int32_t gradient_ok, hessian_ok, gradient_worst_index, hessian_worst_index, nonfinite, pad;
  double gradient_worst_excess, hessian_worst_excess;
};
