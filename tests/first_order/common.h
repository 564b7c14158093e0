// common.h — the C interface shared by the CPU twin (fo_twin.cpp) and the reference harness (ref_harness.cpp): one
// batched GradientDescent / ConjugatedGradientDescent solve on a built-in objective, the stopping fields of
// mi355_lbfgs_stop and the config of mi355_armijo_config, flattened.
#pragma once
#include <cstdint>

extern "C" {
struct fo_stop {  // = mi355_lbfgs_stop
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
struct fo_config {  // = mi355_armijo_config (the reference's constexpr constants; ConjugatedGradientDescent only)
  double c, rho, alpha_min;
};
struct fo_progress {  // = mi355_lbfgs_progress
  int32_t status;
  uint32_t num_iterations;
  uint32_t nfev;
  uint32_t sum_k;
  double x_delta;
  double f_delta;
  double gradient_norm;
};
// what the twin saw on the way, per solve (the golden generator's assertions; not part of the device's output)
struct fo_counters {
  uint32_t max_trials;        // the longest search, in trial points
  uint32_t alpha_one_steps;   // steps that accepted alpha = 1
  uint32_t alpha_less_steps;  // steps that accepted alpha < 1
  uint32_t alpha_min_exits;   // Armijo searches that ended on alpha <= alpha_min with the decrease test still failing
  uint32_t refused_searches;  // More-Thuente searches that refused (dginit >= 0): the step x - g with rate 1
};
}

// methods (= mi355::FirstOrderMethod) and objective ids (= mi355_objective, plus the quartic double well of the
// user-objective example, which reads x_0 alone)
enum { kFoGradientDescent = 0, kFoConjugatedGradientDescent = 1 };
enum { kFoRosenbrock = 0, kFoDiagQuadratic = 1, kFoQuartic = 100 };
