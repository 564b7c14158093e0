// common.h — the C interface shared by the CPU twin (nm_twin.cpp) and the reference harness (ref_harness.cpp): one
// batched NelderMead solve on a built-in objective, the stopping fields of mi355_lbfgs_stop and the config of
// mi355_nelder_mead_config, flattened.
#pragma once
#include <cstdint>

extern "C" {
struct nm_stop {  // = mi355_lbfgs_stop
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
struct nm_config {  // = mi355_nelder_mead_config
  double rho, xi, gamma, sigma, degenerate_tol;
  int32_t mode;  // 0 value (DifferentiabilityMode::None), 1 first
};
struct nm_progress {  // = mi355_lbfgs_progress
  int32_t status;
  uint32_t num_iterations;
  uint32_t nfev;
  uint32_t sum_k;
  double x_delta;
  double f_delta;
  double gradient_norm;
};
// where the per-iteration states of problem 0 go (null = no recording): one row (num_iterations, status, value, x_delta,
// f_delta, gradient_norm) and the iterate per Progress::Update, in order
struct nm_trajectory {
  int32_t capacity;
  int32_t count;
  double* rows;  // [capacity][6]
  double* xs;    // [capacity][n]
};
}

// objective ids (= mi355_objective, plus the value-only l1 + quadratic of the user-objective example)
enum { kNmRosenbrock = 0, kNmDiagQuadratic = 1, kNmL1Quadratic = 100 };
