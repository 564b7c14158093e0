// newton_descent_kernel.hpp — the whole NewtonDescent solve of one problem on one wavefront segment.
//
// Device counterpart of
//   Solver::Minimize                  solver/solver.h:181-224       (driver loop)
//   NewtonDescent::OptimizationStep   solver/newton_descent.h:66-81 (H + 1e-5 I, LU solve, Armijo, x + rate d)
//   Armijo<F, 2>::Search              linesearch/armijo.h:82-102    (the search with the Newton curvature term)
//   Progress::Update                  solver/progress.h:153-327     (solver_driver.hpp, progress_device.hpp)
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
#include "solver_driver.hpp"
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

  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const int n = a.n;
  const bool own = sl < n;
  const bool condition_on = a.hessian_condition_stop > 0.0;
  const long long queue_length = queue_length_of(a);
  const int lds_problem = newton_descent_lds_doubles(n, W, condition_on);
  double* const Hm = lds + seg * lds_problem;
  double* const Am = Hm + n * n;          // H + safe_guard I, then its LU
  double* const vbuf = Am + n * n;
  int* const piv = reinterpret_cast<int*>(vbuf + W);
  double* const hc = vbuf + W + lu_pivot_doubles(n);   // condition_hessian: a copy of H, the column buffers, pivots
  double* const past_f = plateau_ring_slot<W>(a, seg);

  Obj obj;
  obj.load(a.obj_params, n, sl, nullptr, nullptr);

  double x[1], g[1], gt[1], xt[1];
  double f = 0.0;
  SolveProgress prog;                                      // prog.sum_k: the trial evaluations
  long long prob = 0;
  bool need_fetch = true;

  while (true) {
    if (need_fetch) {
      bool drained;
      prob = fetch_problem<W>(a, queue_length, sl, drained);
      if (drained) break;
      x[0] = own ? a.x0[prob * n + sl] : 0.0;
      obj.begin_problem(a.per_problem, prob, a.per_problem_stride, sl);
      need_fetch = false;
      // Solver::Minimize prologue (solver.h:189-192), Progress reset
      f = obj.template eval<W, 1>(x, g, n, sl);
      prog.reset<W, 1>(1, x);
      obj.template hess_full<W, 1>(x, Hm, n, sl);
    }

    // ======================= NewtonDescent::OptimizationStep ==========================
    prog.nfev += 1;                                           // function(current.x, &gradient, &hessian)   (:73)
    // hessian += safe_guard * Identity (:74): every element gets its (rounded) addend, the off-diagonal ones + 0.0
    for (int t = sl; t < n * n; t += W) Am[t] = Hm[t] + 0.0;
    segment_lds_fence();
    if (own) Am[sl * n + sl] = Hm[sl * n + sl] + cfg.safe_guard;
    segment_lds_fence();
    seg_lu_factor<W>(Am, piv, n, sl);                      // hessian.lu()                              (:76)
    double d = seg_lu_solve<W>(Am, piv, -g[0], n, sl);     // .solve(-gradient)
    d = own ? d : 0.0;
    // ---- Armijo<F, 2>::Search (armijo.h:82-102) ------------------------------------------
    prog.nfev += 1;                                           // f_in = function(x, &gradient, &hessian)   (:90)
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
    const double xprev[1] = {x[0]};
    while (ft > fprev + alpha * cache) {                   // (:97-100)
      if (alpha * cfg.armijo_rho == alpha) break;          // the bounded search: see the head of this file
      alpha = alpha * cfg.armijo_rho;
      xt[0] = x[0] + alpha * d;
      ft = obj.template eval<W, 1>(xt, gt, n, sl);
      ++trials;
    }
    prog.nfev += trials + 1;                                  // the trials, and StateType(function, x + rate d) (solver.h)
    prog.sum_k += trials;
    x[0] = xt[0];
    f = ft;
    g[0] = gt[0];

    prog.update<W, 1>(a.stop, a.stop.gradient_norm, true, f, fprev, x, xprev, g, past_f, sl);   // Progress::Update
    // H(x) of the new iterate: the condition test below and the next step
    if (prog.status == MI355_STATUS_CONTINUE) obj.template hess_full<W, 1>(x, Hm, n, sl);
    if (condition_on && prog.status == MI355_STATUS_CONTINUE &&
        hessian_condition_violated<W>(Hm, hc, n, sl, a.hessian_condition_stop))
      prog.status = MI355_STATUS_HESSIAN_CONDITION_VIOLATION;
    trace_iteration<1>(a, prob, n, sl, prog.num_iterations, prog.status, f, prog.x_delta, prog.f_delta,
                       prog.gradient_norm, x, g);
    if (prog.status != MI355_STATUS_CONTINUE) {
      prog.store<1>(a, prob, n, sl, f, x, g, false);
      need_fetch = true;
    }
  }
}

}  // namespace mi355
