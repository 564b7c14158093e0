// newton_descent_kernel.hpp — the whole NewtonDescent solve of one problem on one wavefront segment.
//
// Device counterpart of
//   Solver::Minimize                  solver/solver.h:181-224       (driver loop)
//   NewtonDescent::OptimizationStep   solver/newton_descent.h:66-81 (H + 1e-5 I, LU solve, Armijo, x + rate d)
//   Armijo<F, 2>::Search              linesearch/armijo.h:82-102    (the search with the Newton curvature term)
//   Progress::Update                  solver/progress.h:153-327     (progress_device.hpp)
//
// Mapping.  As the trust-region kernel (trust_region_kernel.hpp): a problem of dimension n <= W is owned by a segment of
// W consecutive lanes, one coordinate per lane; lane j keeps x_j, g_j, d_j in registers.  Per problem the segment's LDS
// holds H(x) (n x n, column major, from the functor's hess_full), a second n x n matrix that becomes H + safe_guard I and
// is factorised in place, W doubles of staging and the pivots.
//   H          built once per iterate.  It serves OptimizationStep's function(x, &g, &H), Armijo's second evaluation at
//              the same x (armijo.h:90) and Progress::Update's condition_hessian test: the repeated calls are counted in
//              nfev, not run.
//   d          seg_lu_factor / seg_lu_solve (lu_device.hpp): PartialPivLU in the pinned order, no reductions.
//   g . d      the segment butterfly (seg_sum).
//   d' H d     armijo.h:93-95 evaluates ((0.5 c) c) d' H d left to right: the row vector (k d)', then
//              v_j = sum_i (k d_i) H(i, j) ascending in i with the first term a product, then sum_j v_j d_j.  Lane j walks
//              down column j of H (stride n across lanes: bank conflicts, accepted — the walk runs once per step; reading
//              the transposed element instead would need a bitwise-symmetric H, which a user functor does not promise);
//              the last sum is the butterfly.
//   trials     eval at x + alpha d.  The step returns x + rate d (newton_descent.h:80): the same expression and bits as the
//              last trial point, so the state rebuild of Solver::Minimize (one more evaluation) is counted, not run —
//              value and gradient of the last trial are kept.
// nfev per step: 1 (OptimizationStep) + 1 (Armijo at x) + the trials + 1 (rebuild); progress.sum_k is the total number of
// trial evaluations.
//
// THE ONE DEPARTURE from the reference: the search is bounded.  `alpha *= 0.9` reaches a fixed point in the denormals
// (2.5e-323, after 7,050 multiplications); where the Armijo condition still fails there (d = +-inf with f = +inf and a
// cache of -inf, say) the reference never returns.  The trial loop here also ends when alpha * rho == alpha, and the step
// proceeds with that alpha.  No status value reports it.
//
// Control flow is uniform over a segment (every scalar comes out of a butterfly or of segment-uniform inputs); different
// segments of a wavefront run different problems (persistent work queue).  Exact arithmetic only (-ffp-contract=off).
#pragma once
#include <stdint.h>

#include "../../include/mi355_lbfgs.h"
#include "hessian_condition_device.hpp"
#include "lbfgs_kernel.hpp"
#include "lu_device.hpp"
#include "newton_descent_config.hpp"
#include "objectives.hpp"
#include "progress_device.hpp"
#include "wave_primitives.hpp"

namespace mi355 {

// LDS doubles one problem needs: H, the regularised copy the LU overwrites, W doubles of staging, the pivots, and
// (condition_hessian test on) the condition computation's region
__host__ __device__ inline int newton_descent_lds_doubles(int n, int W, bool condition) {
  return 2 * n * n + W + lu_pivot_doubles(n) + (condition ? hessian_condition_lds_doubles(n, W) : 0);
}

template <int W, class Obj>
__global__ __launch_bounds__(64) void newton_descent_kernel(const SolveArgs a, const NewtonDescentDeviceConfig cfg) {
  static_assert(Obj::kLdsDoubles == 0 && Obj::shared_lds_doubles() == 0,
                "the Newton-descent kernel is built for functors without LDS data");
  static_assert(HasHessFull<Obj>::value, "the Newton-descent kernel needs the functor's hess_full");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int kSegs = kWave / W;
  constexpr double eps = 2.220446049250313e-16;

  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const int n = a.n;
  const bool own = sl < n;
  const bool condition_on = a.hessian_condition_stop > 0.0;
  const long long queue_length = a.count_dev ? static_cast<long long>(*a.count_dev) : a.B;
  const int lds_problem = newton_descent_lds_doubles(n, W, condition_on);
  double* const Hm = lds + seg * lds_problem;
  double* const Am = Hm + n * n;          // H + safe_guard I, then its LU
  double* const vbuf = Am + n * n;
  int* const piv = reinterpret_cast<int*>(vbuf + W);
  double* const hc = vbuf + W + lu_pivot_doubles(n);   // condition_hessian: a copy of H, the column buffers, pivots
  // plateau ring of stop.past > 0: one MAX_PAST slot per resident segment in global scratch
  double* const past_f =
      a.scratch + (static_cast<size_t>(blockIdx.x) * kSegs + seg) * MI355_LBFGS_MAX_PAST;

  Obj obj;
  obj.load(a.obj_params, n, sl, nullptr, nullptr);

  double x[1], g[1], gt[1], xt[1];
  double f = 0.0;
  unsigned nfev = 0, trials_total = 0, num_iterations = 0;
  int x_delta_violations = 0, f_delta_violations = 0, status = MI355_STATUS_NOT_STARTED;
  double x_delta = 0.0, f_delta = 0.0, gradient_norm = 0.0, xinf_bound = 0.0;
  bool past_init = false;
  int past_pos = 0;
  long long prob = 0;
  bool need_fetch = true;

  while (true) {
    if (need_fetch) {
      // ---- next unsolved problem from the queue ---------------------------------
      unsigned long long nxt = 0;
      if (sl == 0) nxt = atomicAdd(a.next_problem, 1ULL);
      const unsigned lo = static_cast<unsigned>(seg_bcast_first<W>(static_cast<int>(nxt & 0xffffffffULL)));
      const unsigned hi = static_cast<unsigned>(seg_bcast_first<W>(static_cast<int>(nxt >> 32)));
      prob = static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo);
      if (prob >= queue_length) break;
      if (a.problem_map != nullptr) prob = a.problem_map[prob];
      x[0] = own ? a.x0[prob * n + sl] : 0.0;
      obj.begin_problem(a.per_problem, prob, a.per_problem_stride, sl);
      need_fetch = false;
      // Solver::Minimize prologue (solver.h:189-192), Progress reset
      f = obj.template eval<W, 1>(x, g, n, sl);
      nfev = 1;
      trials_total = 0;
      num_iterations = 0;
      x_delta_violations = f_delta_violations = 0;
      x_delta = f_delta = gradient_norm = 0.0;
      status = MI355_STATUS_NOT_STARTED;
      past_init = false;
      past_pos = 0;
      xinf_bound = seg_amax<W, 1>(x);
      obj.template hess_full<W, 1>(x, Hm, n, sl);
    }

    // ======================= NewtonDescent::OptimizationStep ==========================
    nfev += 1;                                             // function(current.x, &gradient, &hessian)   (:73)
    // hessian += safe_guard * Identity (:74): every element gets its (rounded) addend, the off-diagonal ones + 0.0
    for (int t = sl; t < n * n; t += W) Am[t] = Hm[t] + 0.0;
    segment_lds_fence();
    if (own) Am[sl * n + sl] = Hm[sl * n + sl] + cfg.safe_guard;
    segment_lds_fence();
    seg_lu_factor<W>(Am, piv, n, sl);                      // hessian.lu()                              (:76)
    double d = seg_lu_solve<W>(Am, piv, -g[0], n, sl);     // .solve(-gradient)
    d = own ? d : 0.0;
    // ---- Armijo<F, 2>::Search (armijo.h:82-102) ------------------------------------------
    nfev += 1;                                             // f_in = function(x, &gradient, &hessian)   (:90)
    double alpha = 1.0;
    xt[0] = x[0] + alpha * d;
    double ft = obj.template eval<W, 1>(xt, gt, n, sl);    // function(x + alpha d)                     (:91)
    unsigned trials = 1;
    const double gd = seg_sum<W>(g[0] * d);
    const double kq = (0.5 * cfg.armijo_c) * cfg.armijo_c;
    vbuf[sl] = kq * d;
    segment_lds_fence();
    double v = 0.0;
    if (own) {
      const double* const col = Hm + sl * n;
      v = vbuf[0] * col[0];
      for (int i = 1; i < n; ++i) v = v + vbuf[i] * col[i];
    }
    segment_lds_fence();
    const double cache = cfg.armijo_c * gd + seg_sum<W>(v * d);   // (:92-95)
    const double fprev = f;
    const double xprev = x[0];
    while (ft > fprev + alpha * cache) {                   // (:97-100)
      if (alpha * cfg.armijo_rho == alpha) break;          // the bounded search: see the head of this file
      alpha = alpha * cfg.armijo_rho;
      xt[0] = x[0] + alpha * d;
      ft = obj.template eval<W, 1>(xt, gt, n, sl);
      ++trials;
    }
    nfev += trials + 1;                                    // the trials, and StateType(function, x + rate d) (solver.h)
    trials_total += trials;
    x[0] = xt[0];
    f = ft;
    g[0] = gt[0];

    // ========================== Progress::Update ============================
    num_iterations++;                                      // :188
    f_delta = __builtin_fabs(f - fprev);                   // :189
    double dx[1] = {x[0] - xprev};
    x_delta = seg_amax<W, 1>(dx);                          // :190
    gradient_norm = seg_amax<W, 1>(g);                     // :195
    xinf_bound = (xinf_bound + x_delta) * (1.0 + 4.0 * eps);
    status = progress_stop_tests<W, 1>(a.stop, a.stop.num_iterations, a.stop.gradient_norm, num_iterations, f, fprev,
                                       x_delta, f_delta, gradient_norm, xinf_bound, x, x_delta_violations,
                                       f_delta_violations, past_f, past_init, past_pos, sl);
    // H(x) of the new iterate: the condition test below and the next step
    if (status == MI355_STATUS_CONTINUE) obj.template hess_full<W, 1>(x, Hm, n, sl);
    if (condition_on && status == MI355_STATUS_CONTINUE) {  // :318-325, ||H|| ||H^-1|| at current_x (:203-210)
      for (int t = sl; t < n * n; t += W) hc[t] = Hm[t];
      segment_lds_fence();
      const double condition =
          seg_hessian_condition<W>(hc, hc + n * n, reinterpret_cast<int*>(hc + n * n + W * (n + 1)), n, sl);
      if (condition > a.hessian_condition_stop) status = MI355_STATUS_HESSIAN_CONDITION_VIOLATION;
    }
    trace_iteration<1>(a, prob, n, sl, num_iterations, status, f, x_delta, f_delta, gradient_norm, x, g);
    if (status != MI355_STATUS_CONTINUE) {
      // ---- results of this problem (solver.h:223) ---------------------------
      if (own) {
        a.x_out[prob * n + sl] = x[0];
        if (a.g_out) a.g_out[prob * n + sl] = g[0];
      }
      if (sl == 0) {
        a.f_out[prob] = f;
        if (a.progress_out) {
          mi355_lbfgs_progress pr;
          pr.status = status;
          pr.num_iterations = num_iterations;
          pr.nfev = nfev;
          pr.sum_k = trials_total;
          pr.x_delta = x_delta;
          pr.f_delta = f_delta;
          pr.gradient_norm = gradient_norm;
          a.progress_out[prob] = pr;
        }
      }
      need_fetch = true;
    }
  }
}

}  // namespace mi355
