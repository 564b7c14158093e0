// derivative_check_kernel.hpp — the derivative checker: the device functor's own gradient and Hessian next to the
// finite-difference ones built from the functor's VALUES, and the two verdicts.
//
// Device counterpart of utils/derivatives.h of the reference, operation for operation:
//   ComputeFiniteGradient   :37-83     dv_gradient_kernel
//   ComputeFiniteHessian    :86-252    dv_finite_hessian_kernel
//   IsGradientCorrect       :254-280   dv_compare_kernel on (grad, grad_fd)
//   IsHessianCorrect        :282-311   dv_hessian_kernel (function(x, nullptr, &H)) and dv_compare_kernel on (hess, hess_fd)
// run on what a solve actually evaluates: the hand-written HIP functor (eval / value / hess_full), not the host operator().
//
// Mapping.  As the solvers: a point of dimension n <= W * E is owned by a segment of W consecutive lanes, coordinate
// j = sl * E + e in lane sl.  Every evaluation of the functor is made by the whole segment; the lane that owns the
// perturbed coordinate changes its register, everyone else passes x through.  The function value comes out of the
// functor's own reduction (the in-lane tree, then seg_sum), so it is segment-uniform and every lane accumulates the same
// stencil sum; the owner of the coordinate (lane 0 of the segment for a Hessian entry) writes the result.
//   dv_gradient_kernel        one item per point: eval -> grad, value -> f, then the n coordinates one after the other
//   dv_hessian_kernel         one item per point, E = 1: hess_full -> the segment's LDS (n x n, column major) -> global
//   dv_finite_hessian_kernel  one item per (point, row i), E = 1: f0, the diagonal entry and every j > i (4 or 16 values
//                             per pair); writes (i, j) and (j, i).  Each item computes f0 itself: the same bits each time
//   dv_compare_kernel         one 64-lane workgroup per point, no functor: the verdict, the worst excess, the count
// Every item does the same fixed amount of work: plain one-shot grids, no work queue.
//
// Padding.  Padding coordinates hold 0 and never write.  Padding segments (items past the end) run the whole item at
// x = 0 and write nothing, so a wavefront-wide operation inside a functor (the fences of a hess_full, a butterfly) is
// reached by every lane.  In the row kernel the number of columns j > i differs between the segments of a wavefront:
// all of them run to the largest count among the wavefront's items and the extra trips are masked.
//
// Arithmetic.  h = step * max(|x_d|, 1) with step = sqrt(eps) = 2^-26 unless overridden; std::max(a, b) is (a < b) ? b : a,
// NaN behaviour included.  The sums start at 0 and add weight * f in stencil order; one division at the end.  Exact
// arithmetic only (-ffp-contract=off).
//
// Verdicts.  The reference's test |a - e| > tol * max(max(|a|, |e|), 1) with tol the FLOAT constant widened to double.
// A NaN on either side makes the comparison false: the entry PASSES, as in the reference (reproduced, not repaired); so
// does an infinite entry (inf > inf is false).  Such entries — either side NaN or infinite — are counted in `nonfinite`.
// excess = |a - e| / (tol * scale); the worst one and the index of its first occurrence are reported (entries whose
// excess is NaN take no part; no comparable entry: excess 0, index -1).
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "../../include/mi355_lbfgs.h"
#include "derivative_check_config.hpp"
#include "first_order_kernel.hpp"   // HasValueOnly
#include "lbfgs_kernel.hpp"         // HasHessFull, segment_lds_fence
#include "objectives.hpp"
#include "wave_primitives.hpp"

namespace mi355 {

// does the functor evaluate value and gradient?  (a value-only functor, as examples/user_objective_l1, does not.)  Asked
// from host code too (the launch refuses what a functor lacks), so the test names the member, as HasHessFull does: a
// test that CALLS a __device__ member gives another answer where it is first instantiated from a host function.
template <class Obj, int W, int E, class = void>
struct HasEval : std::false_type {};
template <class Obj, int W, int E>
struct HasEval<Obj, W, E, std::void_t<decltype(&Obj::template eval<W, E>)>> : std::true_type {};

// f(x): the functor's value() where it has one, else eval with the gradient dropped
template <int W, int E, class Obj>
__device__ __forceinline__ double dv_value(const Obj& obj, const double (&x)[E], int n, int sl) {
  if constexpr (HasValueOnly<Obj, W, E>::value) {
    return obj.template value<W, E>(x, n, sl);
  } else {
    double g[E];
    return obj.template eval<W, E>(x, g, n, sl);
  }
}

// std::max(a, b)
__device__ __forceinline__ double dv_max(double a, double b) { return (a < b) ? b : a; }
__device__ __forceinline__ double dv_step(double factor, double xd) {
  return factor * dv_max(__builtin_fabs(xd), 1.0);
}

// utils/derivatives.h:52-63: weights, offsets (in units of h) and the divisor of the 2, 4, 6, 8 point stencils
__device__ constexpr double kDvWeight[4][8] = {{1, -1, 0, 0, 0, 0, 0, 0},
                                               {1, -8, 8, -1, 0, 0, 0, 0},
                                               {-1, 9, -45, 45, -9, 1, 0, 0},
                                               {3, -32, 168, -672, 672, -168, 32, -3}};
__device__ constexpr double kDvOffset[4][8] = {{1, -1, 0, 0, 0, 0, 0, 0},
                                               {-2, -1, 1, 2, 0, 0, 0, 0},
                                               {-3, -2, -1, 1, 2, 3, 0, 0},
                                               {-4, -3, -2, -1, 1, 2, 3, 4}};
__device__ constexpr double kDvDivisor[4] = {2, 12, 60, 840};

template <int W, int E, class Obj>
__global__ __launch_bounds__(64) void dv_gradient_kernel(const DerivativeArgs a) {
  static_assert(Obj::kLdsDoubles == 0 && Obj::shared_lds_doubles() == 0,
                "the derivative checker is built for functors without LDS data");
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const int n = a.n;
  const long long item = static_cast<long long>(blockIdx.x) * kSegs + seg;
  const bool active = item < a.B;
  const long long point = active ? item : 0;

  Obj obj;
  obj.load(a.obj_params, n, sl, nullptr, nullptr);
  obj.begin_problem(a.per_problem, point, a.per_problem_stride, sl);

  double x[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = sl * E + e;
    x[e] = (active && j < n) ? a.x[point * n + j] : 0.0;
  }
  if constexpr (HasEval<Obj, W, E>::value) {
    if (a.grad_out != nullptr) {   // (kernel argument: uniform)
      double g[E];
      (void)obj.template eval<W, E>(x, g, n, sl);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = sl * E + e;
        if (active && j < n) a.grad_out[point * n + j] = g[e];
      }
    }
  }
  if (a.f_out != nullptr) {
    const double f = dv_value<W, E, Obj>(obj, x, n, sl);
    if (active && sl == 0) a.f_out[point] = f;
  }
  if (a.grad_fd_out == nullptr) return;

  // ---- ComputeFiniteGradient (:65-82) ------------------------------------------------
  const int acc = a.gradient_accuracy;
  const int inner_steps = 2 * (acc + 1);
  for (int d = 0; d < n; ++d) {
    double h[E];   // of the lane's own coordinates; only the owner of d uses its entry
#pragma unroll
    for (int e = 0; e < E; ++e) h[e] = dv_step(a.gradient_step, x[e]);
    double sum = 0.0;
    for (int s = 0; s < inner_steps; ++s) {
      const double offset = kDvOffset[acc][s];
      double xp[E];
#pragma unroll
      for (int e = 0; e < E; ++e) xp[e] = (sl * E + e == d) ? x[e] + offset * h[e] : x[e];
      const double fv = dv_value<W, E, Obj>(obj, xp, n, sl);
      sum = sum + kDvWeight[acc][s] * fv;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (active && sl * E + e == d) a.grad_fd_out[point * n + d] = sum / (kDvDivisor[acc] * h[e]);
    }
  }
}

template <int W, class Obj>
__global__ __launch_bounds__(64) void dv_hessian_kernel(const DerivativeArgs a) {
  static_assert(Obj::kLdsDoubles == 0 && Obj::shared_lds_doubles() == 0,
                "the derivative checker is built for functors without LDS data");
  static_assert(HasHessFull<Obj>::value, "the analytic-Hessian kernel needs the functor's hess_full");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const int n = a.n;
  const long long item = static_cast<long long>(blockIdx.x) * kSegs + seg;
  const bool active = item < a.B;
  const long long point = active ? item : 0;
  double* const Hm = lds + seg * n * n;

  Obj obj;
  obj.load(a.obj_params, n, sl, nullptr, nullptr);
  obj.begin_problem(a.per_problem, point, a.per_problem_stride, sl);
  double x[1];
  x[0] = (active && sl < n) ? a.x[point * n + sl] : 0.0;
  obj.template hess_full<W, 1>(x, Hm, n, sl);
  segment_lds_fence();
  if (active) {
    double* const out = a.hess_out + point * n * n;
    for (int t = sl; t < n * n; t += W) out[t] = Hm[t];
  }
}

// the sixteen points of :167-241 in the reference's order: four terms of four values; offsets of x_i and x_j in units of
// h, and whether the value is added to or subtracted from its term
__device__ constexpr double kDvCi[16] = {1, 2, -2, -1, -1, -2, 1, 2, 2, -2, -2, 2, -1, 1, 1, -1};
__device__ constexpr double kDvCj[16] = {-2, -1, 1, 2, -2, -1, 2, 1, -2, 2, -2, 2, -1, 1, -1, 1};
__device__ constexpr int kDvMinus[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 1};

template <int W, class Obj>
__global__ __launch_bounds__(64) void dv_finite_hessian_kernel(const DerivativeArgs a) {
  static_assert(Obj::kLdsDoubles == 0 && Obj::shared_lds_doubles() == 0,
                "the derivative checker is built for functors without LDS data");
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const int n = a.n;
  const long long total = a.B * n;
  const long long first_item = static_cast<long long>(blockIdx.x) * kSegs;
  const long long item = first_item + seg;
  const bool active = item < total;
  const long long point = active ? item / n : 0;
  const int i = active ? static_cast<int>(item % n) : 0;
  // the columns j > i of the wavefront's longest row: every segment runs that many trips (wavefront-uniform)
  int trips = 0;
  for (int s = 0; s < kSegs; ++s) {
    const long long it = first_item + s;
    const int cols = (it < total) ? n - 1 - static_cast<int>(it % n) : 0;
    trips = (cols > trips) ? cols : trips;
  }

  Obj obj;
  obj.load(a.obj_params, n, sl, nullptr, nullptr);
  obj.begin_problem(a.per_problem, point, a.per_problem_stride, sl);
  double x[1], xp[1];
  x[0] = (active && sl < n) ? a.x[point * n + sl] : 0.0;
  double* const out = a.hess_fd_out + point * n * n;

  const double f0 = dv_value<W, 1, Obj>(obj, x, n, sl);                      // :104
  const double hi = dv_step(a.hessian_step, seg_coordinate<W, 1>(x, i, sl));  // :110-111, :149-150
  xp[0] = (sl == i) ? x[0] + hi : x[0];
  const double f_plus = dv_value<W, 1, Obj>(obj, xp, n, sl);
  xp[0] = (sl == i) ? x[0] - hi : x[0];
  const double f_minus = dv_value<W, 1, Obj>(obj, xp, n, sl);
  const double diag = (f_plus - 2.0 * f0 + f_minus) / (hi * hi);            // :119, :157
  if (active && sl == 0) out[static_cast<long long>(i) * n + i] = diag;

  for (int t = 1; t <= trips; ++t) {
    const bool valid = i + t < n;
    const int j = valid ? i + t : i;   // (a masked trip perturbs x_i twice and writes nothing)
    const double hj = dv_step(a.hessian_step, seg_coordinate<W, 1>(x, j, sl));
    double entry;
    if (a.hessian_accuracy == 0) {
      // :125-141 (x[i] += hi then x[j] += hj on a copy of x0)
      double fc[4];
#pragma unroll 1
      for (int k = 0; k < 4; ++k) {
        double v = x[0];
        if (sl == i) v = (k < 2) ? v + hi : v - hi;
        if (sl == j) v = ((k & 1) == 0) ? v + hj : v - hj;
        xp[0] = v;
        fc[k] = dv_value<W, 1, Obj>(obj, xp, n, sl);
      }
      entry = (fc[0] - fc[1] - fc[2] + fc[3]) / (4.0 * hi * hj);
    } else {
      // :162-246
      const double h = (hi + hj) / 2.0;
      double term[4];
      for (int q = 0; q < 4; ++q) {
        double tsum = 0.0;
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
          const int k = q * 4 + r;
          double v = x[0];
          if (sl == i) v = x[0] + kDvCi[k] * h;
          if (sl == j) v = x[0] + kDvCj[k] * h;   // (i == j on a masked trip only)
          xp[0] = v;
          const double fv = dv_value<W, 1, Obj>(obj, xp, n, sl);
          tsum = kDvMinus[k] ? tsum - fv : tsum + fv;
        }
        term[q] = tsum;
      }
      entry = (-63.0 * term[0] + 63.0 * term[1] + 44.0 * term[2] + 74.0 * term[3]) / (600.0 * h * h);
    }
    if (active && valid && sl == 0) {
      out[static_cast<long long>(j) * n + i] = entry;   // (i, j), column major
      out[static_cast<long long>(i) * n + j] = entry;   // (j, i): a copy
    }
  }
}

// One 64-lane workgroup per point.  Lanes walk the entries with stride 64 and keep their own worst excess (first index on
// a tie, since a lane's indices ascend); the lanes are then merged pairwise, larger excess first, smaller index on a tie.
// (a template so that the units that include this header do not each define the symbol)
template <bool kHessian>
__global__ __launch_bounds__(64) void dv_compare_kernel(const DerivativeCompareArgs c) {
  const int lane = threadIdx.x;
  const long long point = blockIdx.x;
  const double* const act = c.actual + point * c.count;
  const double* const exp = c.expected + point * c.count;
  double worst = -1.0;
  int worst_index = 0x7fffffff;
  int failed = 0, nonfinite = 0;
  for (int t = lane; t < c.count; t += kWave) {
    const double av = act[t], ev = exp[t];
    const double aa = __builtin_fabs(av), ae = __builtin_fabs(ev);
    const double scale = dv_max(dv_max(aa, ae), 1.0);
    const double diff = __builtin_fabs(av - ev);
    const double bound = c.tol * scale;
    if (diff > bound) failed = 1;
    if (!(aa < __builtin_inf()) || !(ae < __builtin_inf())) ++nonfinite;
    const double excess = diff / bound;
    if (excess > worst) {
      worst = excess;
      worst_index = t;
    }
  }
  for (int off = kWave / 2; off >= 1; off >>= 1) {
    const double ow = __shfl_xor(worst, off, kWave);
    const int oi = __shfl_xor(worst_index, off, kWave);
    failed |= __shfl_xor(failed, off, kWave);
    nonfinite += __shfl_xor(nonfinite, off, kWave);
    if (ow > worst || (ow == worst && oi < worst_index)) {
      worst = ow;
      worst_index = oi;
    }
  }
  if (lane == 0) {
    mi355_derivative_report* const r = c.report + point;
    const bool none = worst < 0.0;
    if constexpr (kHessian) {
      r->hessian_ok = failed ? 0 : 1;
      r->hessian_worst_index = none ? -1 : worst_index;
      r->hessian_worst_excess = none ? 0.0 : worst;
      r->nonfinite += nonfinite;
    } else {
      r->gradient_ok = failed ? 0 : 1;
      r->gradient_worst_index = none ? -1 : worst_index;
      r->gradient_worst_excess = none ? 0.0 : worst;
      r->nonfinite += nonfinite;
    }
  }
}

}  // namespace mi355
