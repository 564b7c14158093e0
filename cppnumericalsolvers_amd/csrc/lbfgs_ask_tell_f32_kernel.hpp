// lbfgs_ask_tell_f32_kernel.hpp — Lbfgs<F, m, MoreThuente>::Minimize with ScalarType = float in reverse communication:
// the float solver state of every problem lives in HBM between calls, one kernel call advances every problem up to its
// next objective evaluation, and the CALLER evaluates the batch of float trial points and hands float f, g back.
//
// The phase machine is that of lbfgs_ask_tell_kernel.hpp; the STATEMENTS are those of lbfgs_f32_kernel.hpp and of the
// float mt_cvsrch / mt_cstep (more_thuente_device.hpp; the search cut at its evaluation is MtSearch<float> of the same
// header) on the same operands in the same order, cut at the objective evaluation, so a callback that
// evaluates with the library's own float functor reproduces the persistent float kernel bit for bit.  What that means
// against the fp64 ask/tell kernel:
//   * s.y is stored per ring slot, not 1 / (s.y); the |s.y| < eps skip is a real skip and rho = one / denom is formed
//     inside both loops of the recursion;
//   * the pair test s.y > eps ||s|| ||y|| is evaluated as written; there is no bound shortcut and no running bound on
//     ||x||_inf;
//   * every constant is static_cast<float>(double literal); the thresholds of the stop record arrive converted once;
//   * the three doubles of the progress record are the float values widened, a NaN among the results is the canonical
//     quiet NaN (CanonicalNan, applied by the shared result gather);
//   * exact arithmetic only (the unit is built with -ffp-contract=off).
//
// Mapping: one problem per segment of W lanes, lane sl owns coordinates sl * E + e; every reduction is a segment
// butterfly of wave_primitives_f32.hpp.  A workgroup is one wavefront; the grid strides over the batch.  A lane reads and
// writes its own 4 E contiguous bytes of a state vector, a segment P * 4 contiguous bytes.  Scalars are read by every lane
// (one address per segment) and written by lane 0.
//
// One call does a bounded amount of work per problem: at most one post-evaluation part of the search, one update (s, y,
// pair test, ring push, gamma, Progress::Update) and one direction (two passes over mem_count <= m slots).  No loop
// waits for a stopping test.  A search that is refused at once (dginit >= 0, more_thuente.h:152-156) costs one round
// without an evaluation: the next call runs that iteration's update whatever the caller's f / g rows hold.
#pragma once
#include <limits>

#include "lbfgs_ask_tell_f32_config.hpp"
#include "lbfgs_f32_kernel.hpp"
#include "wave_primitives_f32.hpp"
#include "ask_tell_kernel_common.hpp"

namespace mi355 {
namespace ask_tell_f32 {

// lane 0's LDS / state scalars are read by the other lanes of its segment
__device__ __forceinline__ void segment_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One step of problem `prob` on the calling segment.  `slot`: its row of the caller's arrays (x_eval, f, g) — `prob`
// itself, or its place in the list of a compacted handle (ask_tell_compact_kernel.hpp); everything else is indexed by
// `prob`.  sy_l / alpha_l: MI355_LBFGS_MAX_M floats of LDS of this segment.  Returns whether the problem is still
// active after the call.
template <int W, int E>
__device__ __forceinline__ bool step_problem(const Args& a, long long prob, long long slot, int sl, float* sy_l,
                                             float* alpha_l) {
  using namespace f32;
  constexpr int P = W * E;
  const float eps = std::numeric_limits<float>::epsilon();
  const float zero = static_cast<float>(0), one = static_cast<float>(1);

  Scalars* const sc = a.scalars + prob;
  const int phase = sc->phase;
  if (phase == kPhaseFinished) return false;

  const int n = a.n, m = a.m;
  float* const row = a.vectors + prob * row_floats(m, P) + sl * E;
  float* const xs = row;
  float* const gs = row + P;
  float* const ds = row + 2 * P;
  float* const Ss = row + 3 * P;
  float* const Ys = Ss + static_cast<long long>(m) * P;
  const long long base = slot * n + sl * E;  // of the caller's [B][n] arrays

  float x[E], g[E], d[E];
  float f = zero, scaling_factor = one, x_delta = zero, f_delta = zero, gradient_norm = zero;
  int mem_count = 0, mem_pos = 0, status = MI355_STATUS_NOT_STARTED, x_delta_violations = 0, f_delta_violations = 0;
  int past_pos = 0;
  bool past_init = false;
  unsigned nfev = 0, sum_k = 0, num_iterations = 0;

  MtSearch<float> mt;  // the running search, segment-uniform
  // the trial point wa + stp s = x - stp d into the evaluation buffer, and the search's scalars
  auto ask_trial = [&]() {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (sl * E + e < n) a.x_eval[base + e] = x[e] - mt.stp * d[e];
    if (sl == 0) {
      mt.store(sc);
      sc->nfev = nfev;
      sc->phase = kPhaseTrial;
    }
  };
  // what Progress and the solver keep across iterations
  auto store_iteration_scalars = [&](int next_phase) {
    if (sl == 0) {
      sc->f = f; sc->scaling_factor = scaling_factor;
      sc->x_delta = x_delta; sc->f_delta = f_delta; sc->gradient_norm = gradient_norm;
      sc->mem_count = mem_count; sc->mem_pos = mem_pos; sc->status = status;
      sc->x_delta_violations = x_delta_violations; sc->f_delta_violations = f_delta_violations;
      sc->past_init = past_init; sc->past_pos = past_pos;
      sc->nfev = nfev; sc->sum_k = sum_k; sc->num_iterations = num_iterations;
      sc->phase = next_phase;
    }
  };

  if (phase == kPhaseFirst) {
    // ---- Solver::Minimize prologue (solver.h:189-194): the caller's f, g are the evaluation at x0 ----------------
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const bool in = sl * E + e < n;
      x[e] = in ? a.x_eval[base + e] : zero;
      g[e] = in ? a.g[base + e] : zero;
    }
    f = a.f[slot];
    nfev = 1;  // the fetch of lbfgs_f32_kernel.hpp: everything else is the initial value above
#pragma unroll
    for (int e = 0; e < E; ++e) {
      xs[e] = x[e];
      gs[e] = g[e];
    }
  } else {
    float xp[E], gp[E];  // the state the search started from
#pragma unroll
    for (int e = 0; e < E; ++e) {
      xp[e] = xs[e];
      gp[e] = gs[e];
    }
    const float fprev = sc->f;
    scaling_factor = sc->scaling_factor;
    mem_count = sc->mem_count; mem_pos = sc->mem_pos;
    x_delta_violations = sc->x_delta_violations; f_delta_violations = sc->f_delta_violations;
    past_init = sc->past_init != 0; past_pos = sc->past_pos;
    nfev = sc->nfev; sum_k = sc->sum_k; num_iterations = sc->num_iterations;
    for (int i = sl; i < m; i += W) sy_l[i] = sc->sy[i];
    segment_fence();
    if (phase == kPhaseTrial) {
      // ---- the cvsrch loop body after the evaluation (more_thuente.h:200-252) --------------------------------------
#pragma unroll
      for (int e = 0; e < E; ++e) {
        d[e] = ds[e];
        g[e] = (sl * E + e < n) ? a.g[base + e] : zero;
      }
      f = a.f[slot];
      mt.load(sc);
      // (g.s is reduced ahead of the search's own statements here and handed in as a value: the float step kernel ran
      // longer with the reduction inside them, the fp64 kernels longer without — profiles/ask_tell_refactor_ab.txt)
      nfev++;
      const float dg = -seg_dot<W, E>(g, d);
      if (mt.after_evaluation(f, [dg]() { return dg; }) == 0) {
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = xp[e];
        ask_trial();
        return true;
      }
      // the search ended: the accepted point, re-formed from the accepted step (as f32::mt_cvsrch ends)
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = xp[e] - mt.stp * d[e];
    } else {
      // ---- no evaluation wanted: the refused search left x, f, g untouched ------------------------------------------
#pragma unroll
      for (int e = 0; e < E; ++e) {
        x[e] = xp[e];
        g[e] = gp[e];
      }
      f = fprev;
    }

    // ---- after the search (lbfgs_f32_kernel.hpp: non-finite bail-out, s, y, pair test, ring push, gamma) -------------
    if (!__builtin_isfinite(f)) {  // return current (lbfgs.h:239-241)
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
          Ss[static_cast<long long>(slot) * P + e] = sv[e];
          Ys[static_cast<long long>(slot) * P + e] = yv[e];
        }
        if (sl == 0) {
          sy_l[slot] = sy;
          sc->sy[slot] = sy;
        }
        segment_fence();
      }
      if (yy > eps) {  // :289-298
        const float temp_scaling = sy / yy;
        if (__builtin_isfinite(temp_scaling) && __builtin_fabsf(temp_scaling) <= static_cast<float>(1e7))
          scaling_factor = fmax_std(temp_scaling, eps);
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = (sl * E + e < n) ? x[e] : zero;  // (a NaN step times 0 on a padding coordinate)

    // ---- Progress::Update (progress.h:188-317), the statements of lbfgs_f32_kernel.hpp --------------------------------
    num_iterations++;                      // :188
    f_delta = __builtin_fabsf(f - fprev);  // :189
    {
      float dx[E];
#pragma unroll
      for (int e = 0; e < E; ++e) dx[e] = x[e] - xp[e];
      x_delta = seg_amax<W, E>(dx);        // :190
    }
    gradient_norm = seg_amax<W, E>(g);     // :195
    const mi355_lbfgs_stop& st = a.stop;
    status = MI355_STATUS_CONTINUE;
    bool decided = false;
    if ((st.num_iterations > 0) && (num_iterations > st.num_iterations)) {  // :212-216
      status = MI355_STATUS_ITERATION_LIMIT;
      decided = true;
    }
    if (!decided) {  // :254-262
      if ((a.stop_x_delta > zero) && (x_delta < a.stop_x_delta)) {
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
      if ((a.stop_f_delta > zero) && (f_delta < a.stop_f_delta * fscale)) {
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
      float* const past_f = sc->past_f;
      if (!past_init) {
        if (sl < p) past_f[sl] = f;  // ring lazily filled with the current f
        past_init = true;
        past_pos = 0;
        segment_fence();
      }
      if (static_cast<int>(num_iterations) > p) {
        const float pf = past_f[past_pos];
        const float rate = __builtin_fabsf(pf - f) / fmax_std(one, __builtin_fabsf(f));
        if (rate < a.stop_past_delta) {
          status = MI355_STATUS_F_DELTA_VIOLATION;
          decided = true;
        }
      }
      if (!decided) {
        if (sl == 0) past_f[past_pos] = f;
        segment_fence();
        past_pos = (past_pos + 1 == p) ? 0 : past_pos + 1;
      }
    }
    if (!decided && a.stop_gradient_norm > zero) {  // :299-317
      const float scale = st.gradient_norm_relative ? fmax_std(one, seg_amax<W, E>(x)) : one;
      if (gradient_norm < a.stop_gradient_norm * scale) status = MI355_STATUS_GRADIENT_NORM_VIOLATION;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      xs[e] = x[e];
      gs[e] = g[e];
    }
    if (status != MI355_STATUS_CONTINUE) {
      // finished: frozen from here on; the evaluation buffer holds the returned x
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (sl * E + e < n) a.x_eval[base + e] = canonical_nan(x[e]);
      store_iteration_scalars(kPhaseFinished);
      return false;
    }
  }

  // ======================= Lbfgs::OptimizationStep up to the search (lbfgs.h:89-232) =====================================
#pragma unroll
  for (int e = 0; e < E; ++e) d[e] = g[e];  // :145
  const int k = mem_count;
  sum_k += k;
  {
    const bool full = (mem_count >= m);
    // chronological position i lives in slot i while the ring fills, in slot (mem_pos + i) mod m once it is full (:162)
    auto slot_of = [&](int i) {
      int idx = full ? mem_pos + i : i;
      return (idx >= m) ? idx - m : idx;
    };
    // first loop, newest -> oldest (:157-171)
    for (int i = k - 1; i >= 0; --i) {
      const int slot = slot_of(i);
      const float denom = sy_l[slot];
      if (__builtin_fabsf(denom) < eps) continue;
      const float rho = one / denom;
      float sv[E], yv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        sv[e] = Ss[static_cast<long long>(slot) * P + e];
        yv[e] = Ys[static_cast<long long>(slot) * P + e];
      }
      const float alpha = rho * seg_dot<W, E>(sv, d);
      if (sl == 0) alpha_l[i] = alpha;
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = d[e] - alpha * yv[e];
    }
#pragma unroll
    for (int e = 0; e < E; ++e) d[e] = d[e] * scaling_factor;  // :181
    segment_fence();
    // second loop, oldest -> newest (:185-196)
    for (int i = 0; i < k; ++i) {
      const int slot = slot_of(i);
      const float denom = sy_l[slot];
      if (__builtin_fabsf(denom) < eps) continue;
      const float rho = one / denom;
      float sv[E], yv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        sv[e] = Ss[static_cast<long long>(slot) * P + e];
        yv[e] = Ys[static_cast<long long>(slot) * P + e];
      }
      const float beta = rho * seg_dot<W, E>(yv, d);
      const float c = alpha_l[i] - beta;
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = d[e] + sv[e] * c;
    }
    segment_fence();  // (sy_l and alpha_l are rewritten by the next problem of this segment)
  }
  const float descent_direction = -seg_dot<W, E>(g, d);  // :199; also cvsrch's dginit = g.s with s = -d
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
    const float gnorm = __builtin_sqrtf(gg);
    alpha_init = (gnorm > eps) ? one / gnorm : one;
    dginit = gg;  // s = -d = g: the search sees g.g >= 0 and returns at once (quirk Q1)
  }
#pragma unroll
  for (int e = 0; e < E; ++e) ds[e] = d[e];

  if (dginit >= zero) {  // more_thuente.h:152-156: no evaluation; the next call finishes this iteration
    store_iteration_scalars(kPhaseNoEval);
    return true;
  }
  // ---- the search starts (more_thuente.h:158-177) and asks for its first trial -----------------------------------------
  store_iteration_scalars(kPhaseTrial);
  mt.start(f, dginit, alpha_init);
  ask_trial();
  return true;
}

// static LDS of a step kernel, per segment: s.y per ring slot and the alpha of the running recursion
constexpr int kSyLds = MI355_LBFGS_MAX_M, kAlphaLds = MI355_LBFGS_MAX_M;
template <int W>
constexpr int step_lds_bytes() {
  return (kWave / W) * (kSyLds + kAlphaLds) * static_cast<int>(sizeof(float));
}

// One step of every row a.B counts, and the tally of the problems still active after it.  Dense (kListed false): row
// r is problem r and a.B the batch.  Listed: row s of x_eval / f / g belongs to problem ids[s], ids ascending, a.B is
// the LENGTH OF THE LIST (nothing of a step is indexed by the batch size) and the grid is sized from it.  (Why the grid
// loop is spelled here and not in a function the three paths share: run_steps of lbfgsb_ask_tell_kernel.hpp.)
template <int W, int E, bool kListed>
__device__ __forceinline__ void run_steps(const Args a, const long long* ids) {
  constexpr int kSegs = kWave / W;
  __shared__ float sy_lds[kSegs][kSyLds];
  __shared__ float alpha_lds[kSegs][kAlphaLds];
  static_assert(sizeof(sy_lds) + sizeof(alpha_lds) == step_lds_bytes<W>(), "what the launch reports");
  const int lane = threadIdx.x;
  const int seg = lane / W;
  const int sl = lane % W;
  unsigned long long active_count = 0;  // wavefront-uniform
  const long long stride = static_cast<long long>(gridDim.x) * kSegs;
  for (long long first = static_cast<long long>(blockIdx.x) * kSegs; first < a.B; first += stride) {
    const long long slot = first + seg;
    bool active = false;
    if (slot < a.B) active = step_problem<W, E>(a, kListed ? ids[slot] : slot, slot, sl, sy_lds[seg], alpha_lds[seg]);
    active_count += __builtin_popcountll(__builtin_amdgcn_ballot_w64(active && sl == 0));
  }
  if (lane == 0 && active_count != 0) atomicAdd(a.active, active_count);
}

// The two entry points of run_steps: two kernels, so that the dense one takes no list argument and tests none.
template <int W, int E>
__global__ __launch_bounds__(64) void step_kernel(const Args a) {
  run_steps<W, E, false>(a, nullptr);
}

template <int W, int E>
__global__ __launch_bounds__(64) void listed_step_kernel(const Args a, const long long* ids) {
  run_steps<W, E, true>(a, ids);
}

// How the result gather (ask_tell_kernel_common.hpp) finishes a value, as the persistent float kernel returns them: the
// three doubles of the progress record are the float values widened, every NaN is the canonical quiet NaN.  (The state
// initialisation is ask_tell_kernel_common.hpp's too.)
struct CanonicalNan {
  __device__ static float value(float v) { return f32::canonical_nan(v); }
  __device__ static double widened(float v) { return f32::canonical_nan_widened(v); }
};

}  // namespace ask_tell_f32
}  // namespace mi355
