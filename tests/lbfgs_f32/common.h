// common.h — the C interface shared by the float L-BFGS twin (f32_twin.cpp) and the reference harness (ref_harness.cpp):
// one batched Lbfgs<F, m, MoreThuente> solve with ScalarType = float on a built-in objective, with the stopping fields
// of mi355_lbfgs_stop and the progress record of mi355_lbfgs_progress, flattened.
#pragma once
#include <cstdint>

extern "C" {
struct l32_stop {  // = mi355_lbfgs_stop
  uint64_t num_iterations;
  double x_delta;
  int32_t x_delta_violations;
  double f_delta;
  int32_t f_delta_violations;
  int32_t f_delta_relative;
  double gradient_norm;
  int32_t gradient_norm_relative;
  int32_t past;
  double past_delta;
};
struct l32_progress {  // = mi355_lbfgs_progress (the three doubles: float values widened)
  int32_t status;
  uint32_t num_iterations;
  uint32_t nfev;
  uint32_t sum_k;
  double x_delta;
  double f_delta;
  double gradient_norm;
};
}

// objective ids (= mi355_objective); DiagQuadratic's parameters are n + 1 doubles (a, c), converted to float once
enum { kL32Rosenbrock = 0, kL32DiagQuadratic = 1 };
// per-iteration rows: num_iterations, status, value, x_delta, f_delta, gradient_norm (floats widened to double)
enum { kL32RowWidth = 6 };
