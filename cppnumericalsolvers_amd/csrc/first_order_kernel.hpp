// first_order_kernel.hpp — the whole GradientDescent / ConjugatedGradientDescent solve of one problem on one wavefront
// segment.
//
// Device counterpart of
//   Solver::Minimize                             solver/solver.h:181-224                    (driver loop, state rebuild)
//   GradientDescent::OptimizationStep            solver/gradient_descent.h:64-73            (Method 0)
//   MoreThuente<F, 1>::Search (scalar overload)  linesearch/more_thuente.h:63-77, :137-256  (more_thuente_device.hpp)
//   ConjugatedGradientDescent::InitializeSolver / OptimizationStep
//                                                solver/conjugated_gradient_descent.h:62-85 (Method 1)
//   Armijo<F, 1>::Search                         linesearch/armijo.h:45-64
//   Progress::Update                             solver/progress.h:153-327                  (solver_driver.hpp)
//
// Mapping.  A problem of dimension n <= W * E is owned by a segment of W consecutive lanes, E coordinates per lane
// (coordinate j = sl * E + e, as the Lbfgs kernels); x, g, d and the previous iterate are registers.  No per-problem LDS.
// Inner products are the in-lane tree followed by the segment butterfly (seg_dot).  The padding coordinates hold x = 0,
// g = 0, d = 0 at every point of the solve, so they add zeros to every sum and maximum.
//
// Method 0.  g at the iterate is held; the search direction is s = -g and mt_cvsrch already runs along the negated
// vector it is handed, so it is called with d = g, dginit = -(g.g) and alpha_init = 1.  The step returns x - rate g
// (gradient_descent.h:72): where the search ran, the expression and bits of cvsrch's last trial point, whose value and
// gradient are kept — the state rebuild of Solver::Minimize (solver.h:210-216) is counted, not run.  Where cvsrch
// refuses (dginit >= 0: g.g underflowed to 0) rate stays 1, x - g has not been evaluated and the rebuild runs.
// Method 1.  d = -g at the first step, else beta = (g.g) / (g_prev.g_prev) and d_j = (-g_j) + (beta d_j), two rounded
// operations; a zero denominator gives the reference's inf / NaN.  g_prev.g_prev is the g.g of the step before (the same
// vector, the same sum: the same bits).  The Armijo trials need the value only: functors with a value() run it and one
// eval follows at the accepted point (the rebuild, run for real); with cfg.eval_trials, or without a value(), the
// trials run eval and the last trial's gradient is kept (the rebuild counted).  Either way f and g are the bits of one
// evaluation at x + alpha d.  The search is bounded by alpha > alpha_min (176 trials at the defaults).
// nfev per step: 1 (OptimizationStep) + 1 (the search's evaluation at x) + the trials + 1 (rebuild); the prologue adds 1
// and Method 1's InitializeSolver 1 more.  progress.sum_k is the total number of trial evaluations.
//
// NaN results.  The sign and payload of a NaN belong to the processor and to the order in which the compiler places the
// operands of an addition, not to the reference: an overflowing start (inf - inf in the objective) ends in NaNs whose bits
// differ between this kernel and any host computation of the same operations.  The results of a problem (x, f, g and the
// three progress doubles) are therefore written with every NaN replaced by the one quiet NaN 0x7ff8000000000000; values
// that are not NaN are written as computed.  The trace records are not touched.
//
// Control flow is uniform over a segment (every scalar comes out of a butterfly or of segment-uniform inputs); different
// segments of a wavefront run different problems (persistent work queue).  Exact arithmetic only (-ffp-contract=off).
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "../../include/mi355_lbfgs.h"
#include "first_order_config.hpp"
#include "lbfgs_kernel.hpp"
#include "more_thuente_device.hpp"
#include "objectives.hpp"
#include "solver_driver.hpp"
#include "wave_primitives.hpp"

namespace mi355 {

// does the functor offer the value alone?  (optional member: template <int W, int E> double value(x, n, sl))
template <class Obj, int W, int E, class = void>
struct HasValueOnly : std::false_type {};
template <class Obj, int W, int E>
struct HasValueOnly<Obj, W, E,
                    std::void_t<decltype(std::declval<const Obj&>().template value<W, E>(
                        std::declval<const double (&)[E]>(), 0, 0))>> : std::true_type {};

template <int W, int E, int Method, class Obj>
__global__ __launch_bounds__(64) void first_order_kernel(const SolveArgs a, const FirstOrderDeviceConfig cfg) {
  static_assert(Obj::kLdsDoubles == 0 && Obj::shared_lds_doubles() == 0,
                "the first-order kernel is built for functors without LDS data");
  static_assert(Method == kGradientDescent || Method == kConjugatedGradientDescent, "Method");

  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const int n = a.n;
  const long long queue_length = queue_length_of(a);
  double* const past_f = plateau_ring_slot<W>(a, seg);

  Obj obj;
  obj.load(a.obj_params, n, sl, nullptr, nullptr);

  double x[E], g[E], d[E], xprev[E];
  double f = 0.0, gg_prev = 0.0;
  SolveProgress prog;                                      // prog.sum_k: the trial evaluations
  long long prob = 0;
  bool need_fetch = true;

  while (true) {
    if (need_fetch) {
      bool drained;
      prob = fetch_problem<W>(a, queue_length, sl, drained);
      if (drained) break;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = sl * E + e;
        x[e] = (j < n) ? a.x0[prob * n + j] : 0.0;
        d[e] = 0.0;
      }
      obj.begin_problem(a.per_problem, prob, a.per_problem_stride, sl);
      need_fetch = false;
      // Solver::Minimize prologue (solver.h:189-192), Progress reset
      f = obj.template eval<W, E>(x, g, n, sl);
      // Method 1: InitializeSolver evaluates function(x0, &previous_gradient_) (:62-65): counted, the gradient is g
      prog.reset<W, E>((Method == kConjugatedGradientDescent) ? 2 : 1, x);
      gg_prev = 0.0;
    }

    const double fprev = f;
#pragma unroll
    for (int e = 0; e < E; ++e) xprev[e] = x[e];
    unsigned trials = 0;
    prog.nfev += 2;   // function(current.x, &gradient) of OptimizationStep, and the search's own evaluation at x
    const double gg = seg_dot<W, E>(g, g);
    if constexpr (Method == kGradientDescent) {
      // ================ GradientDescent::OptimizationStep (gradient_descent.h:64-73) ================
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = g[e];   // cvsrch overwrites g; the search runs along -d
      trials = static_cast<unsigned>(mt_cvsrch<W, E, Obj>(obj, x, f, g, 1.0, d, -gg, n, sl));
      if (trials == 0) {
        // the refused search (more_thuente.h:152-156): rate = alpha_init = 1, x - rate g is a new point
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = x[e] - 1.0 * d[e];
        f = obj.template eval<W, E>(x, g, n, sl);   // StateType(function, x) of solver.h:213-214
      }
    } else {
      // ========== ConjugatedGradientDescent::OptimizationStep (conjugated_gradient_descent.h:67-85) ==========
      if (prog.num_iterations == 0) {
#pragma unroll
        for (int e = 0; e < E; ++e) d[e] = -g[e];
      } else {
        const double beta = gg / gg_prev;
#pragma unroll
        for (int e = 0; e < E; ++e) d[e] = (-g[e]) + (beta * d[e]);
      }
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = (sl * E + e < n) ? d[e] : 0.0;   // (inf * 0 on a padding coordinate)
      gg_prev = gg;
      // ---- Armijo<F, 1>::Search (armijo.h:45-64) ------------------------------------------
      constexpr bool kValue = HasValueOnly<Obj, W, E>::value;
      const bool eval_trials = !kValue || cfg.eval_trials != 0;
      double alpha = 1.0;
      double xt[E], gt[E];
#pragma unroll
      for (int e = 0; e < E; ++e) xt[e] = x[e] + alpha * d[e];
      double ft;
      if constexpr (kValue) {
        if (eval_trials) ft = obj.template eval<W, E>(xt, gt, n, sl);
        else ft = obj.template value<W, E>(xt, n, sl);
      } else {
        ft = obj.template eval<W, E>(xt, gt, n, sl);
      }
      trials = 1;
      const double cache = cfg.armijo_c * seg_dot<W, E>(g, d);
      while ((ft > fprev + alpha * cache) && (alpha > cfg.armijo_alpha_min)) {
        alpha = alpha * cfg.armijo_rho;
#pragma unroll
        for (int e = 0; e < E; ++e) xt[e] = x[e] + alpha * d[e];
        if constexpr (kValue) {
          if (eval_trials) ft = obj.template eval<W, E>(xt, gt, n, sl);
          else ft = obj.template value<W, E>(xt, n, sl);
        } else {
          ft = obj.template eval<W, E>(xt, gt, n, sl);
        }
        ++trials;
      }
      // current.x + rate d (:84) is the last trial point
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = xt[e];
      if (eval_trials) {
        f = ft;
#pragma unroll
        for (int e = 0; e < E; ++e) g[e] = gt[e];
      } else {
        f = obj.template eval<W, E>(x, g, n, sl);   // StateType(function, x): the rebuild, run
      }
    }
    prog.nfev += trials + 1;                                  // the trials, and StateType(function, x) (solver.h:213-214)
    prog.sum_k += trials;
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = (sl * E + e < n) ? x[e] : 0.0;   // (a NaN step times 0 on a padding coordinate)

    prog.update<W, E>(a.stop, a.stop.gradient_norm, true, f, fprev, x, xprev, g, past_f, sl);   // Progress::Update
    trace_iteration<E>(a, prob, n, sl, prog.num_iterations, prog.status, f, prog.x_delta, prog.f_delta,
                       prog.gradient_norm, x, g);
    if (prog.status != MI355_STATUS_CONTINUE) {
      prog.store<E>(a, prob, n, sl, f, x, g, true);   // (every NaN as the canonical one: "NaN results" above)
      need_fetch = true;
    }
  }
}

}  // namespace mi355
