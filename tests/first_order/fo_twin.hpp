// fo_twin.hpp — sequential CPU restatement of GradientDescent (reference solver/gradient_descent.h with the scalar
// overload of linesearch/more_thuente.h) and ConjugatedGradientDescent (solver/conjugated_gradient_descent.h with
// linesearch/armijo.h's Armijo<F, 1>) under Solver::Minimize and Progress::Update, in two summation orders:
//   kRefOrder     inner products and the objective's sum are ascending chains over n, as the reference computes them
//                 over the Eigen stand-in: bit for bit the reference;
//   kDeviceOrder  they are the pairwise trees over the zero-padded width W x E of the kernel (csrc/first_order_kernel.hpp:
//                 the in-lane tree over a lane's E consecutive coordinates, then the segment butterfly over the W lanes —
//                 one pairwise tree over W x E positions): bit for bit the device.
// The objectives, the summation policies, cvsrch / cstep and Progress::Update are the ones of oracle/lbfgs_oracle.hpp
// (pinned against the reference on their own); what is stated here is the two solvers' steps, the Armijo search, the
// state rebuild of Solver::Minimize and the count of objective calls.  The twin evaluates the returned point of every
// step for real (the rebuild), where the kernel keeps the last trial's value and gradient: that the two agree is part of
// what the device comparison shows.  In device order the results (x, f, g, the three progress doubles) are written as the
// kernel writes them: every NaN as the one quiet NaN 0x7ff8000000000000 (the sign and payload of a NaN are the
// processor's; csrc/first_order_kernel.hpp, "NaN results"); in reference order they are the host's own bits, as the
// reference harness's are.  Built with -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../oracle/lbfgs_oracle.hpp"
#include "common.h"

namespace fo_twin {

enum Order { kRefOrder = 0, kDeviceOrder = 1 };

// f = (x_0^2 - 2)^2 in n dimensions (examples/user_objective_quartic): t = x x - 2, f = t t, g_0 = (4 x) t
struct Quartic final : oracle::Objective {
  double eval(const double* x, double* g, int n, const oracle::Reducer&) const override {
    const double t = x[0] * x[0] - 2.0;
    for (int i = 0; i < n; ++i) g[i] = 0.0;
    g[0] = (4.0 * x[0]) * t;
    return t * t;
  }
};

// trajectory (may be null): per Progress::Update one row (num_iterations, status, value, x_delta, f_delta,
// gradient_norm) and the iterate, at most `capacity` of them
struct Trajectory {
  int capacity;
  double* rows;
  double* xs;
  int count;
};

struct Step {
  std::vector<double> x;  // the returned point
  uint32_t trials;
};

// GradientDescent::OptimizationStep (gradient_descent.h:64-73)
inline Step gradient_descent_step(const oracle::Objective& obj, const oracle::Reducer& red, const oracle::State& cur,
                                  fo_counters& cnt) {
  const int n = static_cast<int>(cur.x.size());
  const std::vector<double>& gradient = cur.gradient;   // function(current.x, &gradient): the bits of the state's
  std::vector<double> s(n), g = gradient, xx = cur.x;
  for (int i = 0; i < n; ++i) s[i] = -gradient[i];
  double alpha = 1.0, f = cur.value;                    // Search (:63-77): f, g = function(x, &g), alpha_init = 1
  uint64_t trials = 0;
  oracle::MoreThuente::cvsrch(obj, red, &xx, &f, &g, &alpha, s, &trials);
  if (trials == 0) ++cnt.refused_searches;
  if (alpha == 1.0) ++cnt.alpha_one_steps;
  if (alpha < 1.0) ++cnt.alpha_less_steps;
  Step out{std::vector<double>(n), static_cast<uint32_t>(trials)};
  for (int i = 0; i < n; ++i) out.x[i] = cur.x[i] - alpha * gradient[i];   // :72
  return out;
}

// ConjugatedGradientDescent::OptimizationStep (conjugated_gradient_descent.h:67-85) with Armijo<F, 1>::Search
// (armijo.h:45-64)
struct ConjugateState {
  std::vector<double> previous_gradient, search_direction;
};
inline Step conjugated_gradient_step(const oracle::Objective& obj, const oracle::Reducer& red, const fo_config& c,
                                     const oracle::State& cur, uint64_t num_iterations, ConjugateState& cs,
                                     fo_counters& cnt) {
  const int n = static_cast<int>(cur.x.size());
  const std::vector<double>& g = cur.gradient;
  if (num_iterations == 0) {
    cs.search_direction.assign(n, 0.0);
    for (int i = 0; i < n; ++i) cs.search_direction[i] = -g[i];
  } else {
    const double beta = red.dot(g.data(), g.data(), n) /
                        red.dot(cs.previous_gradient.data(), cs.previous_gradient.data(), n);
    for (int i = 0; i < n; ++i) cs.search_direction[i] = (-g[i]) + (beta * cs.search_direction[i]);
  }
  cs.previous_gradient = g;
  const std::vector<double>& d = cs.search_direction;
  double alpha = 1.0;
  const double f_in = cur.value;
  std::vector<double> xt(n), gt(n);
  for (int i = 0; i < n; ++i) xt[i] = cur.x[i] + alpha * d[i];
  double f = obj.eval(xt.data(), gt.data(), n, red);
  uint32_t trials = 1;
  const double cache = c.c * red.dot(g.data(), d.data(), n);
  while (f > f_in + alpha * cache && alpha > c.alpha_min) {
    alpha *= c.rho;
    for (int i = 0; i < n; ++i) xt[i] = cur.x[i] + alpha * d[i];
    f = obj.eval(xt.data(), gt.data(), n, red);
    ++trials;
  }
  if (!(alpha > c.alpha_min) && f > f_in + alpha * cache) ++cnt.alpha_min_exits;
  if (alpha == 1.0) ++cnt.alpha_one_steps;
  if (alpha < 1.0) ++cnt.alpha_less_steps;
  Step out{std::vector<double>(n), trials};
  for (int i = 0; i < n; ++i) out.x[i] = cur.x[i] + alpha * d[i];   // :84
  return out;
}

// Solver::Minimize (solver.h:181-224)
inline void solve_one(int method, const oracle::Objective& obj, int n, Order order, int width, const fo_stop& st,
                      const fo_config& c, const double* x0, double* x_out, double* f_out, double* g_out,
                      fo_progress* prog, fo_counters* counters, Trajectory* traj = nullptr) {
  oracle::Reducer red;
  red.kind = (order == kDeviceOrder) ? oracle::Reduction::Butterfly : oracle::Reduction::Sequential;
  red.width = width;
  oracle::Stopping stop;
  stop.num_iterations = st.num_iterations;
  stop.x_delta = st.x_delta;
  stop.x_delta_violations = st.x_delta_violations;
  stop.f_delta = st.f_delta;
  stop.f_delta_violations = st.f_delta_violations;
  stop.f_delta_relative = st.f_delta_relative != 0;
  stop.gradient_norm = st.gradient_norm;
  stop.gradient_norm_relative = st.gradient_norm_relative != 0;
  stop.past = st.past;
  stop.past_delta = st.past_delta;
  fo_counters cnt{0, 0, 0, 0, 0};
  oracle::State cur;
  cur.x.assign(x0, x0 + n);
  cur.gradient.assign(n, 0.0);
  cur.value = obj.eval(cur.x.data(), cur.gradient.data(), n, red);   // StateType(function, x0) (:191)
  uint32_t nfev = 1, trials_total = 0;
  ConjugateState cs;
  if (method == kFoConjugatedGradientDescent) ++nfev;   // InitializeSolver: function(x0, &previous_gradient_)
  oracle::Progress progress;
  do {
    const oracle::State prev = cur;
    nfev += 2;   // OptimizationStep's function(current.x, &gradient) and the search's evaluation at x
    const Step step = (method == kFoGradientDescent)
                          ? gradient_descent_step(obj, red, prev, cnt)
                          : conjugated_gradient_step(obj, red, c, prev, progress.num_iterations, cs, cnt);
    nfev += step.trials + 1;   // the trials and the rebuild StateType(function, x) (:213-214)
    trials_total += step.trials;
    cnt.max_trials = std::max(cnt.max_trials, step.trials);
    cur.x = step.x;
    cur.value = obj.eval(cur.x.data(), cur.gradient.data(), n, red);
    progress.Update(prev, cur, stop);
    if (traj != nullptr && traj->count < traj->capacity) {
      double* row = traj->rows + 6 * traj->count;
      row[0] = static_cast<double>(progress.num_iterations);
      row[1] = static_cast<double>(static_cast<int>(progress.status));
      row[2] = cur.value;
      row[3] = progress.x_delta;
      row[4] = progress.f_delta;
      row[5] = progress.gradient_norm;
      for (int j = 0; j < n; ++j) traj->xs[traj->count * n + j] = cur.x[j];
      ++traj->count;
    }
  } while (progress.status == oracle::Continue);
  const auto written = [order](double v) {
    return (order == kDeviceOrder && v != v) ? std::numeric_limits<double>::quiet_NaN() : v;
  };
  for (int j = 0; j < n; ++j) {
    x_out[j] = written(cur.x[j]);
    g_out[j] = written(cur.gradient[j]);
  }
  *f_out = written(cur.value);
  prog->status = static_cast<int32_t>(progress.status);
  prog->num_iterations = static_cast<uint32_t>(progress.num_iterations);
  prog->nfev = nfev;
  prog->sum_k = trials_total;
  prog->x_delta = written(progress.x_delta);
  prog->f_delta = written(progress.f_delta);
  prog->gradient_norm = written(progress.gradient_norm);
  if (counters) *counters = cnt;
}

}  // namespace fo_twin
