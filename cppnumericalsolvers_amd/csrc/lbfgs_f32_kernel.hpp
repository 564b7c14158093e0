// lbfgs_f32_kernel.hpp — the whole L-BFGS solve of one problem on one wavefront segment with ScalarType = float.
//
// Device counterpart of the reference's Lbfgs<F, m, MoreThuente> instantiated on a float function:
//   Solver::Minimize            solver/solver.h:181-224   (prologue, driver loop)
//   Lbfgs::InitializeSolver     solver/lbfgs.h:72-87
//   Lbfgs::OptimizationStep     solver/lbfgs.h:89-303     (two-loop recursion, descent check and fallback, alpha_init,
//                                                          line search, pair test, ring push, gamma update)
//   Progress::Update            solver/progress.h:153-327 (every threshold of the stop record converted to float once)
// with f32::mt_cvsrch / mt_cstep<float> from more_thuente_device.hpp.  A file of its own: the fp64 kernels (lbfgs_kernel.hpp) are not
// templated on a scalar type and their object code does not change.
//
// Mapping.  One problem per segment of W lanes, E coordinates per lane, coordinate j = sl * E + e; padding coordinates
// are held at zero.  x, g, d, the previous x / g and every scalar are float registers.  Both halves of the (s, y) history
// are a float ring in LDS, S[slot][sl][e] then Y[slot][sl][e]: 2 m W E floats per segment.  A lane touches only its own
// columns (4 E contiguous bytes at a 4 E byte lane stride: ds_read_b32 / b64 / b128, no bank conflict at any built E), so
// the ring needs no barrier.  Behind the ring sit 2 m segment-uniform floats per segment: s.y of every stored pair (the
// denominator lbfgs.h:163-168 / :187-192 recomputes from the stored columns: the same sum of the same products, the same
// bits) and the alpha_i of the running recursion; they are written by lane 0 of the segment and read by all its lanes
// behind a wavefront fence.  m is a run-time argument.  The plateau ring (stop.past > 0) is the context's global scratch
// slot of the resident segment, holding floats.
//
// Exact arithmetic only: no FMA, no reordering, direct reductions (no running bound on ||x||_inf; the pair test
// evaluates eps ||s|| ||y|| as the reference writes it).  Results: x, f, g as float; the progress record's three doubles
// are the float values widened (exact); a NaN among any of them is written as the canonical quiet NaN.
// Control flow is uniform over a segment; the segments of a wavefront run different problems (persistent work queue of
// solver_driver.hpp) and re-initialise in place.
#pragma once
#include <stdint.h>

#include <limits>

#include "../../include/mi355_lbfgs.h"
#include "lbfgs_f32_config.hpp"
#include "lbfgs_kernel.hpp"
#include "more_thuente_device.hpp"
#include "objectives_f32.hpp"
#include "solver_driver.hpp"
#include "wave_primitives_f32.hpp"

namespace mi355 {
namespace f32 {

__device__ __forceinline__ float canonical_nan(float v) { return (v != v) ? __builtin_nanf("") : v; }
__device__ __forceinline__ double canonical_nan_widened(float v) {
  return (v != v) ? __builtin_nan("") : static_cast<double>(v);
}

template <int W, int E, class Obj>
__global__ __launch_bounds__(64) void lbfgs_f32_kernel(const SolveArgs a, const LbfgsF32Args fa) {
  extern __shared__ __attribute__((aligned(16))) float lds_f32[];
  constexpr int WE = W * E;
  const float eps = std::numeric_limits<float>::epsilon();
  const float zero = static_cast<float>(0), one = static_cast<float>(1);

  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const int n = a.n;
  const int m = a.m;
  const long long queue_length = queue_length_of(a);
  float* const S = lds_f32 + seg * lds_floats_per_problem(m, WE);
  float* const Y = S + m * WE;
  float* const sy_mem = Y + m * WE;      // s.y of the pair in each slot
  float* const alpha_mem = sy_mem + m;   // alpha_i of the running recursion, by chronological position
  float* const past_f = reinterpret_cast<float*>(plateau_ring_slot<W>(a, seg));
  float* const Sl = S + sl * E;
  float* const Yl = Y + sl * E;

  Obj obj;
  obj.load(fa.obj_params, n, sl);

  float x[E], g[E];
  float f = zero;
  unsigned nfev = 0, sum_k = 0, num_iterations = 0;
  int mem_count = 0, mem_pos = 0;
  float scaling_factor = one;
  int x_delta_violations = 0, f_delta_violations = 0;
  float x_delta = zero, f_delta = zero, gradient_norm = zero;
  int status = MI355_STATUS_NOT_STARTED;
  bool past_init = false;
  int past_pos = 0;
  long long prob = 0;
  bool need_fetch = true;
#pragma unroll
  for (int e = 0; e < E; ++e) x[e] = g[e] = zero;

  while (true) {
    if (need_fetch) {
      bool drained;
      prob = fetch_problem<W>(a, queue_length, sl, drained);
      if (drained) break;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = sl * E + e;
        x[e] = (j < n) ? fa.x0[prob * n + j] : zero;
      }
      need_fetch = false;
      // Solver::Minimize prologue (solver.h:189-192), Lbfgs::InitializeSolver (lbfgs.h:84-86), a fresh Progress
      f = obj.template eval<W, E>(x, g, n, sl);
      nfev = 1;
      sum_k = 0;
      mem_count = 0;
      mem_pos = 0;
      scaling_factor = one;
      num_iterations = 0;
      x_delta_violations = f_delta_violations = 0;
      x_delta = f_delta = gradient_norm = zero;
      status = MI355_STATUS_NOT_STARTED;
      past_init = false;
      past_pos = 0;
    }

    // ======================= Lbfgs::OptimizationStep ========================
    float d[E];
#pragma unroll
    for (int e = 0; e < E; ++e) d[e] = g[e];  // :145
    const int k = mem_count;
    sum_k += k;
    const bool full = (mem_count >= m);
    // chronological position i lives in slot i while the ring fills, in slot (mem_pos + i) mod m once it is full (:162)
    auto slot_of = [&](int i) {
      int idx = full ? mem_pos + i : i;
      return (idx >= m) ? idx - m : idx;
    };
    // first loop, newest -> oldest (:157-171)
    for (int i = k - 1; i >= 0; --i) {
      const int slot = slot_of(i);
      const float denom = sy_mem[slot];
      if (__builtin_fabsf(denom) < eps) continue;
      const float rho = one / denom;
      float sv[E], yv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        sv[e] = Sl[slot * WE + e];
        yv[e] = Yl[slot * WE + e];
      }
      const float alpha = rho * seg_dot<W, E>(sv, d);
      if (sl == 0) alpha_mem[i] = alpha;
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = d[e] - alpha * yv[e];
    }
#pragma unroll
    for (int e = 0; e < E; ++e) d[e] = d[e] * scaling_factor;  // :181
    segment_lds_fence();
    // second loop, oldest -> newest (:185-196)
    for (int i = 0; i < k; ++i) {
      const int slot = slot_of(i);
      const float denom = sy_mem[slot];
      if (__builtin_fabsf(denom) < eps) continue;
      const float rho = one / denom;
      float sv[E], yv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        sv[e] = Sl[slot * WE + e];
        yv[e] = Yl[slot * WE + e];
      }
      const float beta = rho * seg_dot<W, E>(yv, d);
      const float c = alpha_mem[i] - beta;
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = d[e] + sv[e] * c;
    }

    const float descent_direction = -seg_dot<W, E>(g, d);  // :199
    // cvsrch's dginit = g.s with s = -d (more_thuente.h:151) is the same number: every product and every partial sum is
    // the exact negation
    float dginit = descent_direction;
    float alpha_init = one;  // :207-213
    if (mem_count == 0) {
      const float dn = __builtin_sqrtf(seg_dot<W, E>(d, d));
      alpha_init = (dn > eps) ? one / dn : one;
    }
    const float relative_eps = eps * fmax_std(one, __builtin_sqrtf(seg_dot<W, E>(x, x)));  // :93-95
    if (!__builtin_isfinite(descent_direction) || descent_direction > -eps * relative_eps) {  // :214-224
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = -g[e];
      mem_count = 0;
      mem_pos = 0;
      const float gg = seg_dot<W, E>(g, g);
      const float gn = __builtin_sqrtf(gg);
      alpha_init = (gn > eps) ? one / gn : one;
      dginit = gg;  // s = -d = g: the line search sees g.g >= 0 and returns at once (quirk Q1)
    }

    // line search along -d (:231-232); the current state is kept for s, y and for the non-finite bail-out (:239-241)
    float xp[E], gp[E];
    const float fprev = f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      xp[e] = x[e];
      gp[e] = g[e];
    }
    nfev += mt_cvsrch<W, E, Obj>(obj, x, f, g, alpha_init, d, dginit, n, sl);

    if (!__builtin_isfinite(f)) {  // return current (:239-241)
      f = fprev;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        x[e] = xp[e];
        g[e] = gp[e];
      }
    } else {
      float sv[E], yv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        sv[e] = x[e] - xp[e];  // :248
        yv[e] = g[e] - gp[e];  // :249
      }
      const float sy = seg_dot<W, E>(sv, yv);  // :265
      const float yy = seg_dot<W, E>(yv, yv);  // :290, and grad_diff.norm()^2 of :266
      const float sy_threshold = eps * __builtin_sqrtf(seg_dot<W, E>(sv, sv)) * __builtin_sqrtf(yy);  // :266
      if (sy > sy_threshold) {  // :267-280
        int slot;
        if (mem_count < m) {
          slot = mem_count;
          mem_count++;
        } else {
          slot = mem_pos;
          mem_pos = (mem_pos + 1 == m) ? 0 : mem_pos + 1;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
          Sl[slot * WE + e] = sv[e];
          Yl[slot * WE + e] = yv[e];
        }
        if (sl == 0) sy_mem[slot] = sy;
        segment_lds_fence();
      }
      if (yy > eps) {  // :289-298 (grad_diff.dot(x_diff): the products commute, the bits of sy)
        const float temp_scaling = sy / yy;
        if (__builtin_isfinite(temp_scaling) && __builtin_fabsf(temp_scaling) <= static_cast<float>(1e7))
          scaling_factor = fmax_std(temp_scaling, eps);
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = (sl * E + e < n) ? x[e] : zero;  // (a NaN step times 0 on a padding coordinate)

    // ========================== Progress::Update ============================
    num_iterations++;                     // :188
    f_delta = __builtin_fabsf(f - fprev);  // :189
    {
      float dx[E];
#pragma unroll
      for (int e = 0; e < E; ++e) dx[e] = x[e] - xp[e];
      x_delta = seg_amax<W, E>(dx);       // :190
    }
    gradient_norm = seg_amax<W, E>(g);    // :195
    const mi355_lbfgs_stop& st = a.stop;
    status = MI355_STATUS_CONTINUE;
    bool decided = false;
    if ((st.num_iterations > 0) && (num_iterations > st.num_iterations)) {  // :212-216
      status = MI355_STATUS_ITERATION_LIMIT;
      decided = true;
    }
    if (!decided) {  // :254-262
      if ((fa.stop_x_delta > zero) && (x_delta < fa.stop_x_delta)) {
        x_delta_violations++;
        if (x_delta_violations >= st.x_delta_violations) {
          status = MI355_STATUS_X_DELTA_VIOLATION;
          decided = true;
        }
      } else {
        x_delta_violations = 0;
      }
    }
    if (!decided) {  // :263-277
      const float fscale =
          st.f_delta_relative ? fmax_std(fmax_std(__builtin_fabsf(f), __builtin_fabsf(fprev)), one) : one;
      if ((fa.stop_f_delta > zero) && (f_delta < fa.stop_f_delta * fscale)) {
        f_delta_violations++;
        if (f_delta_violations >= st.f_delta_violations) {
          status = MI355_STATUS_F_DELTA_VIOLATION;
          decided = true;
        }
      } else {
        f_delta_violations = 0;
      }
    }
    if (!decided && st.past > 0) {  // :280-298
      const int p = st.past;
      if (!past_init) {
        if (sl < p) past_f[sl] = f;  // ring lazily filled with the current f
        past_init = true;
        past_pos = 0;
        segment_lds_fence();
      }
      if (static_cast<int>(num_iterations) > p) {
        const float pf = past_f[past_pos];
        const float rate = __builtin_fabsf(pf - f) / fmax_std(one, __builtin_fabsf(f));
        if (rate < fa.stop_past_delta) {
          status = MI355_STATUS_F_DELTA_VIOLATION;
          decided = true;
        }
      }
      if (!decided) {
        if (sl == 0) past_f[past_pos] = f;
        segment_lds_fence();
        past_pos = (past_pos + 1 == p) ? 0 : past_pos + 1;
      }
    }
    if (!decided && fa.stop_gradient_norm > zero) {  // :299-317
      const float scale = st.gradient_norm_relative ? fmax_std(one, seg_amax<W, E>(x)) : one;
      if (gradient_norm < fa.stop_gradient_norm * scale) status = MI355_STATUS_GRADIENT_NORM_VIOLATION;
    }

    if (status != MI355_STATUS_CONTINUE) {
      // ---- results of this problem (solver.h:223), every NaN as the canonical quiet NaN -----------------------------
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = sl * E + e;
        if (j < n) {
          fa.x_out[prob * n + j] = canonical_nan(x[e]);
          if (fa.g_out) fa.g_out[prob * n + j] = canonical_nan(g[e]);
        }
      }
      if (sl == 0) {
        fa.f_out[prob] = canonical_nan(f);
        if (a.progress_out) {
          mi355_lbfgs_progress pr;
          pr.status = status;
          pr.num_iterations = num_iterations;
          pr.nfev = nfev;
          pr.sum_k = sum_k;
          pr.x_delta = canonical_nan_widened(x_delta);
          pr.f_delta = canonical_nan_widened(f_delta);
          pr.gradient_norm = canonical_nan_widened(gradient_norm);
          a.progress_out[prob] = pr;
        }
      }
      need_fetch = true;
    }
  }
}

// One objective evaluation per row (mi355_lbfgs_eval_batch_f32): row b on segment b % (64 / W) of workgroup b / (64 / W).
template <int W, int E, class Obj>
__global__ __launch_bounds__(64) void eval_f32_kernel(const float* x_in, float* f_out, float* g_out,
                                                      const float* obj_params, long long B, int n) {
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const long long prob = static_cast<long long>(blockIdx.x) * kSegs + seg;
  Obj obj;
  obj.load(obj_params, n, sl);
  if (prob >= B) return;
  float x[E], g[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = sl * E + e;
    x[e] = (j < n) ? x_in[prob * n + j] : 0.0f;
  }
  const float f = obj.template eval<W, E>(x, g, n, sl);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = sl * E + e;
    if (j < n && g_out) g_out[prob * n + j] = g[e];
  }
  if (sl == 0) f_out[prob] = f;
}

}  // namespace f32
}  // namespace mi355
