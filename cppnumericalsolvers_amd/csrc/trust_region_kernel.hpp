// trust_region_kernel.hpp — the whole TrustRegionNewton solve of one problem on one wavefront segment.
//
// Device counterpart of
//   Solver::Minimize                      solver/solver.h:181-224   (driver loop)
//   TrustRegionNewton::OptimizationStep   solver/trust_region_newton.h:190-298 (model, rho, radius, rejection loop)
//   SolveTrustRegionSubproblem            :339-426 (CG-Steihaug)
//   ExtendStepToBoundary                  :436-451
//   Progress::Update                      solver/progress.h:153-327 (solver_driver.hpp, progress_device.hpp)
//
// Mapping.  A problem of dimension n <= W is owned by a segment of W consecutive lanes, one coordinate per lane (E = 1):
// lane j keeps x_j, g_j, and the CG vectors p_j, r_j, d_j in registers.  H(x) is n x n, column major, in the segment's
// LDS, built by the functor's hess_full once per accepted iterate: the reference evaluates H at current.x (:201), and
// that is the x Progress::Update's condition_hessian test reads too (progress.h:203-210), so one H serves the test and
// the next step's model.
//   H d       lane j forms row j as the ascending sequential sum over k of H[j + k n] d_k — the order of the reference's
//             matrix * vector product (ascending, first term a product) — reading consecutive doubles across lanes;
//             d is staged in LDS (W doubles) and read as a broadcast.
//   a . b     the segment butterfly (seg_sum of wave_primitives.hpp): the pairwise tree over the padded width.
// Every scalar of the algorithm comes out of a butterfly or from segment-uniform inputs, so control flow is uniform
// over a segment; different segments of a wavefront run different problems (persistent work queue, as the Lbfgs
// kernels).  Exact arithmetic only (-ffp-contract=off): every a*b+c is a rounded product and a rounded sum.
#pragma once
#include <stdint.h>

#include "../../include/mi355_lbfgs.h"
#include "hessian_condition_device.hpp"
#include "lbfgs_kernel.hpp"
#include "objectives.hpp"
#include "solver_driver.hpp"
#include "trust_region_config.hpp"
#include "wave_primitives.hpp"

namespace mi355 {

// LDS doubles one problem needs: H, the staging vector of H d, and (condition_hessian test on) the LU's region
__host__ __device__ inline int trust_region_lds_doubles(int n, int W, bool condition) {
  return n * n + W + (condition ? hessian_condition_lds_doubles(n, W) : 0);
}

template <int W, class Obj>
__global__ __launch_bounds__(64) void trust_region_kernel(const SolveArgs a, const TrustRegionDeviceConfig cfg) {
  static_assert(Obj::kLdsDoubles == 0 && Obj::shared_lds_doubles() == 0,
                "the trust-region kernel is built for functors without LDS data");
  static_assert(HasHessFull<Obj>::value, "the trust-region kernel needs the functor's hess_full");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr double kInf = __builtin_inf();

  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const int n = a.n;
  const bool own = sl < n;
  const bool condition_on = a.hessian_condition_stop > 0.0;
  const long long queue_length = queue_length_of(a);
  const int lds_problem = trust_region_lds_doubles(n, W, condition_on);
  double* const Hm = lds + seg * lds_problem;
  double* const vbuf = Hm + n * n;
  double* const hc = vbuf + W;            // condition_hessian: a copy of H, the LU's column buffers and pivots
  double* const past_f = plateau_ring_slot<W>(a, seg);

  Obj obj;
  obj.load(a.obj_params, n, sl, nullptr, nullptr);

  // H d: row sl of H against d staged in LDS, ascending over k (the reference's product order)
  auto hess_times = [&](double dj) -> double {
    vbuf[sl] = dj;
    segment_lds_fence();
    double s = 0.0;
    if (own) {
      s = Hm[sl] * vbuf[0];
      for (int k = 1; k < n; ++k) s = s + Hm[sl + k * n] * vbuf[k];
    }
    segment_lds_fence();
    return s;
  };
  auto dot = [&](double u, double v) -> double { return seg_sum<W>(u * v); };

  double x[1], g[1], gt[1], xt[1];
  double f = 0.0, radius = 0.0;
  SolveProgress prog;                                      // prog.sum_k: the CG iterations
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
      // Solver::Minimize prologue (solver.h:189-192), InitializeSolver (:180-187), Progress reset
      f = obj.template eval<W, 1>(x, g, n, sl);
      radius = cfg.initial_radius;
      prog.reset<W, 1>(1, x);
      obj.template hess_full<W, 1>(x, Hm, n, sl);
    }

    // ======================= TrustRegionNewton::OptimizationStep ======================
    prog.nfev += 1;                                           // function(current.x, &gradient, &hessian)   (:201)
    const double gnorm_inf = seg_amax<W, 1>(g);            // :213-214
    const double sq = __builtin_sqrt(gnorm_inf);
    const double forcing = (sq < 0.5) ? sq : 0.5;          // std::min(0.5, sqrt(.)) (:215-216)
    const double cg_tolerance = cfg.cg_forcing_coefficient * forcing * gnorm_inf;  // :217-218
    // :357-358 reads max(dim_, 0) + max(floor, 0), but InitializeSolver (:184-187) sets dim_ and then ResetInternal() zeroes
    // it: the reference's CG cap is the floor alone, reproduced here
    const int cg_max = cfg.cg_extra_iterations;
    const double fprev = f;
    const double xprev[1] = {x[0]};
    bool accepted = false;
    for (int retry = 0; retry < cfg.rejection_retry_limit; ++retry) {
      // ---- CG-Steihaug (:339-426) ----------------------------------------------------
      double p = 0.0, r = g[0], d = -g[0];
      double rr = dot(r, r);
      bool hit = false;
      unsigned cg_iters = 0;
      auto to_boundary = [&]() {                           // ExtendStepToBoundary (:436-451)
        const double qa = dot(d, d);
        const double qb = 2.0 * dot(p, d);
        const double qc = dot(p, p) - radius * radius;
        const double disc = qb * qb - 4.0 * qa * qc;
        const double tau = (-qb + __builtin_sqrt((disc < 0.0) ? 0.0 : disc)) / (2.0 * qa);
        p = p + tau * d;
        hit = true;
      };
      if (!(__builtin_sqrt(rr) <= cg_tolerance)) {         // early exit: the step stays zero (:363-367)
        for (int it = 0; it < cg_max; ++it) {
          ++cg_iters;
          const double hd = hess_times(d);
          const double curvature = dot(d, hd);
          if (!(curvature > 0.0)) {                        // negative / zero / NaN curvature (:376-385)
            to_boundary();
            break;
          }
          const double alpha = rr / curvature;
          const double pc = p + alpha * d;
          if (__builtin_sqrt(dot(pc, pc)) >= radius) {     // :393-397
            to_boundary();
            break;
          }
          p = pc;
          r = r + alpha * hd;
          const double rr_new = dot(r, r);
          if (__builtin_sqrt(rr_new) <= cg_tolerance) break;  // :402-407
          const double beta = rr_new / rr;
          d = -r + beta * d;
          rr = rr_new;
        }
      }
      p = own ? p : 0.0;
      // ---- agreement ratio (:260-280) -------------------------------------------------
      xt[0] = x[0] + p;
      const double trial_value = obj.template eval<W, 1>(xt, gt, n, sl);
      prog.nfev += 1;
      const double hp = hess_times(p);
      const double predicted = -dot(g[0], p) - 0.5 * dot(p, hp);
      const double actual = fprev - trial_value;
      const double rho = (predicted <= 0.0) ? -kInf : actual / predicted;
      // ---- radius (:290-295) ------------------------------------------------------------
      const double radius_before = radius;
      if (rho < cfg.rho_low) {
        radius = radius * cfg.shrink_factor;
      } else if (rho > cfg.rho_high && hit) {
        const double grown = cfg.expand_factor * radius;
        radius = (cfg.max_radius < grown) ? cfg.max_radius : grown;
      }
      prog.sum_k += cg_iters;
      if (rho > cfg.acceptance_threshold) {                // :305-307: StateType(function, trial_x)
        x[0] = xt[0];
        f = trial_value;
        g[0] = gt[0];
        prog.nfev += 1;
        accepted = true;
        break;
      }
      if (radius <= cfg.min_radius) break;                 // :317-319
      if (radius == radius_before) {
        // rho is NaN or between rho_low and the acceptance threshold: the radius stayed put, so every remaining retry
        // solves the identical subproblem and rejects it again — what those retries would add is counted, not re-run
        const unsigned left = static_cast<unsigned>(cfg.rejection_retry_limit - retry - 1);
        prog.nfev += left;
        prog.sum_k += left * cg_iters;
        break;
      }
    }

    prog.update<W, 1>(a.stop, a.stop.gradient_norm, true, f, fprev, x, xprev, g, past_f, sl);   // Progress::Update
    // H(x) of the new iterate (unchanged on a stalled step): the condition test below and the next step's model
    if (accepted && prog.status == MI355_STATUS_CONTINUE) obj.template hess_full<W, 1>(x, Hm, n, sl);
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
