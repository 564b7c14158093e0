// common.h — the C interface shared by the CPU twin (tr_twin.cpp) and the reference harness (ref_harness.cpp): one
// batched TrustRegionNewton solve on a built-in objective, the stopping fields of mi355_lbfgs_stop and the config of
// mi355_trust_region_config, flattened.
#pragma once
#include <cstdint>

extern "C" {
struct tr_stop {  // = mi355_lbfgs_stop
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
struct tr_config {  // = mi355_trust_region_config / TrustRegionNewtonConfig<double>
  double initial_radius, max_radius, acceptance_threshold, shrink_factor, expand_factor, rho_low, rho_high,
      cg_forcing_coefficient;
  int32_t cg_max_iterations_floor;
  double min_radius;
  int32_t rejection_retry_limit;
};
struct tr_progress {  // = mi355_lbfgs_progress
  int32_t status;
  uint32_t num_iterations;
  uint32_t nfev;
  uint32_t sum_k;
  double x_delta;
  double f_delta;
  double gradient_norm;
};
// what the twin saw on the way, per solve (the golden generator's assertions; not part of the device's output)
struct tr_counters {
  uint32_t max_cg_iterations;               // the longest CG-Steihaug run of a subproblem
  uint32_t subproblems_of_3_cg_iterations;  // subproblems that ran at least 3 CG iterations
  uint32_t negative_curvature_exits;        // CG runs that met d'H d <= 0 (or NaN)
  uint32_t boundary_hits;                   // steps extended to the trust-region boundary (either reason)
  uint32_t conditions;                      // condition numbers the stopping test evaluated
  double min_condition_margin;              // the smallest |condition - threshold| / threshold (+inf: none evaluated)
};
}

// objective ids (= mi355_objective, plus the 1-D quartic double well of the user-objective example and the dense quartic
// of examples/user_objective_dense: params = S (n x n, column major), b (n), kappa)
enum { kTrRosenbrock = 0, kTrDiagQuadratic = 1, kTrQuartic = 100, kTrDense = 101 };
