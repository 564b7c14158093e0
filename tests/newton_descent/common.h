// common.h — the C interface shared by the CPU twin (nd_twin.cpp) and the reference harness (ref_harness.cpp): one
// batched NewtonDescent solve on a built-in objective, the stopping fields of mi355_lbfgs_stop and the config of
// mi355_newton_descent_config, flattened.
#pragma once
#include <cstdint>

extern "C" {
struct nd_stop {  // = mi355_lbfgs_stop
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
struct nd_config {  // = mi355_newton_descent_config (the reference's constexpr constants)
  double safe_guard, armijo_c, armijo_rho;
};
struct nd_progress {  // = mi355_lbfgs_progress
  int32_t status;
  uint32_t num_iterations;
  uint32_t nfev;
  uint32_t sum_k;
  double x_delta;
  double f_delta;
  double gradient_norm;
};
// what the twin saw on the way, per solve (the golden generator's assertions; not part of the device's output)
struct nd_counters {
  uint32_t interchanges;      // row interchanges of all the LUs of the solve
  uint32_t max_trials;        // the longest search, in trial points
  uint32_t alpha_one_steps;   // steps that accepted alpha = 1
  uint32_t alpha_less_steps;  // steps that accepted alpha < 1
  uint32_t fixed_point;       // searches that ended because alpha * rho == alpha (the bounded search)
  uint32_t pivot_ties;        // LU columns whose non-zero maximum was attained more than once (the first one is the pivot)
  uint32_t zero_columns;      // LU columns with best == 0 (no interchange, no division; the solve divides by that zero)
  uint32_t conditions;        // condition numbers the stopping test evaluated
  uint32_t pivot_distance[64];  // histogram of p - k over every column of the steps' LUs
  double min_condition_margin;  // the smallest |condition - threshold| / threshold of those (+inf: none evaluated)
};
}
enum { kNdMaxN = 64 };

// objective ids (= mi355_objective, plus the quartic double well of the user-objective example, which reads x_0 alone,
// and the dense quartic of examples/user_objective_dense: params = S (n x n, column major), b (n), kappa)
enum { kNdRosenbrock = 0, kNdDiagQuadratic = 1, kNdQuartic = 100, kNdDense = 101 };
