// solver_driver.hpp — what the TrustRegionNewton, NewtonDescent, NelderMead and first-order kernels share around their
// own algorithm: the work-queue fetch, the running state of Progress::Update (solver/progress.h:153-327) with its reset,
// per-iteration update and write-out, the condition_hessian test of the two Hessian kernels, and the plateau-ring slot.
// Plain __forceinline__ pieces; each kernel keeps its own __global__ function and its own step.  The Lbfgs / Lbfgsb /
// ridge kernels keep their inline statements of the same things (see the head of progress_device.hpp for why).
#pragma once
#include <stdint.h>

#include "../../include/mi355_lbfgs.h"
#include "hessian_condition_device.hpp"
#include "lbfgs_kernel.hpp"
#include "progress_device.hpp"
#include "wave_primitives.hpp"

namespace mi355 {

// the number of queue positions of this launch
__device__ __forceinline__ long long queue_length_of(const SolveArgs& a) {
  return a.count_dev ? static_cast<long long>(*a.count_dev) : a.B;
}

// Next unsolved problem from the work queue, for the segment whose lane `sl` calls: `drained` when the queue holds no
// more, else the problem to work on (queue position q works on problem_map[q] where a map is given).  The problem comes
// back by value: handed out through a reference, the W = 64 first-order kernels took up to three more VGPRs.
template <int W>
__device__ __forceinline__ long long fetch_problem(const SolveArgs& a, long long queue_length, int sl, bool& drained) {
  unsigned long long nxt = 0;
  if (sl == 0) nxt = atomicAdd(a.next_problem, 1ULL);
  const unsigned lo = static_cast<unsigned>(seg_bcast_first<W>(static_cast<int>(nxt & 0xffffffffULL)));
  const unsigned hi = static_cast<unsigned>(seg_bcast_first<W>(static_cast<int>(nxt >> 32)));
  long long prob = static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo);
  drained = prob >= queue_length;
  if (!drained && a.problem_map != nullptr) prob = a.problem_map[prob];
  return prob;
}

// plateau ring of stop.past > 0: one MAX_PAST slot per resident segment in global scratch
template <int W>
__device__ __forceinline__ double* plateau_ring_slot(const SolveArgs& a, int seg) {
  return a.scratch + (static_cast<size_t>(blockIdx.x) * (kWave / W) + seg) * MI355_LBFGS_MAX_PAST;
}

// v, or the canonical quiet NaN where v is one (first_order_kernel.hpp, "NaN results")
__device__ __forceinline__ double canonical_nan(double v) { return (v != v) ? __builtin_nan("") : v; }

// The condition_hessian test (progress.h:318-325, ||H|| ||H^-1|| at current_x :203-210): H (n x n in LDS) is copied to
// the `hc` region (the copy the LU overwrites, then the column buffers and the pivots) and its condition number compared.
template <int W>
__device__ __forceinline__ bool hessian_condition_violated(const double* Hm, double* hc, int n, int sl, double stop) {
  for (int t = sl; t < n * n; t += W) hc[t] = Hm[t];
  segment_lds_fence();
  const double condition =
      seg_hessian_condition<W>(hc, hc + n * n, reinterpret_cast<int*>(hc + n * n + W * (n + 1)), n, sl);
  return condition > stop;
}

// Running state of Progress between the iterations of one solve (segment-uniform values).
struct SolveProgress {
  unsigned nfev = 0, sum_k = 0, num_iterations = 0;
  int x_delta_violations = 0, f_delta_violations = 0, status = MI355_STATUS_NOT_STARTED;
  double x_delta = 0.0, f_delta = 0.0, gradient_norm = 0.0, xinf_bound = 0.0;
  bool past_init = false;
  int past_pos = 0;

  // the start of a solve at x, after `nfev0` evaluations
  template <int W, int E>
  __device__ __forceinline__ void reset(unsigned nfev0, const double (&x)[E]) {
    nfev = nfev0;
    sum_k = 0;
    num_iterations = 0;
    x_delta_violations = f_delta_violations = 0;
    x_delta = f_delta = gradient_norm = 0.0;
    status = MI355_STATUS_NOT_STARTED;
    past_init = false;
    past_pos = 0;
    xinf_bound = seg_amax<W, E>(x);
  }

  // Progress::Update after the step xprev, fprev -> x, f (gradient g): sets status.  `stop_gradient_norm` is the bound of
  // the gradient test (0 = off); with_gradient false leaves gradient_norm as it is (NelderMead's value mode forms no g).
  // The condition_hessian test is the caller's, after this.
  template <int W, int E>
  __device__ __forceinline__ void update(const mi355_lbfgs_stop& stop, double stop_gradient_norm, bool with_gradient,
                                         double f, double fprev, const double (&x)[E], const double (&xprev)[E],
                                         const double (&g)[E], double* past_f, int sl) {
    constexpr double eps = 2.220446049250313e-16;
    num_iterations++;                                      // :188
    f_delta = __builtin_fabs(f - fprev);                   // :189
    double dx[E];
#pragma unroll
    for (int e = 0; e < E; ++e) dx[e] = x[e] - xprev[e];
    x_delta = seg_amax<W, E>(dx);                          // :190
    if (with_gradient) gradient_norm = seg_amax<W, E>(g);  // :193-196
    xinf_bound = (xinf_bound + x_delta) * (1.0 + 4.0 * eps);
    status = progress_stop_tests<W, E>(stop, stop.num_iterations, stop_gradient_norm, num_iterations, f, fprev, x_delta,
                                       f_delta, gradient_norm, xinf_bound, x, x_delta_violations, f_delta_violations,
                                       past_f, past_init, past_pos, sl);
  }

  // results of the problem (solver.h:223).  canonical_nans: every stored double goes through canonical_nan
  template <int E>
  __device__ __forceinline__ void store(const SolveArgs& a, long long prob, int n, int sl, double f, const double (&x)[E],
                                        const double (&g)[E], bool canonical_nans) const {
    auto out = [&](double v) { return canonical_nans ? canonical_nan(v) : v; };
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = sl * E + e;
      if (j < n) {
        a.x_out[prob * n + j] = out(x[e]);
        if (a.g_out) a.g_out[prob * n + j] = out(g[e]);
      }
    }
    if (sl == 0) {
      a.f_out[prob] = out(f);
      if (a.progress_out) {
        mi355_lbfgs_progress pr;
        pr.status = status;
        pr.num_iterations = num_iterations;
        pr.nfev = nfev;
        pr.sum_k = sum_k;
        pr.x_delta = out(x_delta);
        pr.f_delta = out(f_delta);
        pr.gradient_norm = out(gradient_norm);
        a.progress_out[prob] = pr;
      }
    }
  }
};

}  // namespace mi355
