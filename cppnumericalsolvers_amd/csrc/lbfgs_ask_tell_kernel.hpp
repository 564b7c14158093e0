// lbfgs_ask_tell_kernel.hpp — Lbfgs<F, m, MoreThuente>::Minimize in reverse communication: the solver state of every
// problem lives in HBM between calls, one kernel call advances every problem up to its next objective evaluation, and
// the CALLER evaluates the batch of trial points (torch ops, autograd, its own kernels) and hands f, g back.
//
// Device counterpart of the same reference code as lbfgs_kernel.hpp (Solver::Minimize solver/solver.h:181-224,
// Lbfgs::OptimizationStep solver/lbfgs.h:89-303, MoreThuente::cvsrch linesearch/more_thuente.h:137-256,
// Progress::Update solver/progress.h:153-327), cut at the objective evaluation: the statements are those of
// lbfgs_kernel.hpp and mt_cvsrch (more_thuente_device.hpp; the search cut at its evaluation is MtSearch<double> of the
// same header) on the same operands in the same order, so a callback that evaluates with the library's own
// functor reproduces the persistent exact kernel bit for bit.
//
// Mapping: one problem per segment of W lanes, lane sl owns coordinates sl * E + e; every reduction is a segment
// butterfly of wave_primitives.hpp (the pairwise tree over P = W * E, zero padded).  A workgroup is one wavefront; the
// grid strides over the batch.  A lane reads and writes its own 8 E contiguous bytes of a state vector, a segment
// P * 8 contiguous bytes.  Scalars are read by every lane (one address per segment) and written by lane 0.
//
// One call does a bounded amount of work per problem, in this order:
//   trial pending:   the part of the cvsrch loop body after the evaluation; info == 0: the part before the next
//                    evaluation, the trial point into x_eval, return
//   search ended / no evaluation wanted: s, y, pair test, ring push, gamma, Progress::Update and the stopping tests
//   going on (also after the first evaluation): two-loop recursion from the rings, descent test with fallback,
//                    alpha_init; then the first trial point of the next search — or, where that search is refused at
//                    once (dginit >= 0, more_thuente.h:152-156), the phase "no evaluation wanted": the next call runs
//                    that iteration's update (x, f, g unchanged) whatever the caller's f / g rows hold.
// No loop depends on a stopping test firing: the two-loop recursion runs mem_count <= m trips.
#pragma once
#include "lbfgs_ask_tell_config.hpp"
#include "more_thuente_device.hpp"
#include "progress_device.hpp"
#include "wave_primitives.hpp"
#include "ask_tell_kernel_common.hpp"

namespace mi355 {
namespace ask_tell {

// lane 0's LDS scalars are read by the other lanes of its segment (lbfgs_kernel.hpp, segment_lds_fence)
__device__ __forceinline__ void segment_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One step of problem `prob` on the calling segment.  `slot`: its row of the caller's arrays (x_eval, f, g) — `prob`
// itself, or its place in the list of a compacted handle (ask_tell_compact_kernel.hpp); everything else is indexed by
// `prob`.  rho_l / alpha_l: MI355_LBFGS_MAX_M (+ 1) doubles of LDS of this segment.  Returns whether the problem is
// still active after the call.
template <int W, int E>
__device__ __forceinline__ bool step_problem(const Args& a, long long prob, long long slot, int sl, double* rho_l,
                                             double* alpha_l) {
  using AR = ArithExact;
  constexpr int P = W * E;
  constexpr double eps = 2.220446049250313e-16;  // numeric_limits<double>::epsilon()

  Scalars* const sc = a.scalars + prob;
  const int phase = sc->phase;
  if (phase == kPhaseFinished) return false;

  const int n = a.n, m = a.m;
  const double n_as_double = static_cast<double>(n);
  double* const row = a.vectors + prob * row_doubles(m, P) + sl * E;
  double* const xs = row;
  double* const gs = row + P;
  double* const ds = row + 2 * P;
  double* const Ss = row + 3 * P;
  double* const Ys = Ss + static_cast<long long>(m) * P;
  const long long base = slot * n + sl * E;  // of the caller's [B][n] arrays

  double x[E], g[E], d[E];
  double f = 0.0, scaling_factor = 1.0, xinf_bound = 0.0, x_delta = 0.0, f_delta = 0.0, gradient_norm = 0.0;
  int mem_count = 0, mem_pos = 0, status = MI355_STATUS_NOT_STARTED, x_delta_violations = 0, f_delta_violations = 0;
  int past_pos = 0;
  bool past_init = false;
  unsigned nfev = 0, sum_k = 0, num_iterations = 0;

  MtSearch<double> mt;  // the running search, segment-uniform
  // the trial point wa + stp s = x - stp d into the evaluation buffer, and the search's scalars
  auto ask_trial = [&]() {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (sl * E + e < n) a.x_eval[base + e] = AR::nmadd(mt.stp, d[e], x[e]);
    if (sl == 0) {
      mt.store(sc);
      sc->nfev = nfev;
      sc->phase = kPhaseTrial;
    }
  };
  // what Progress and the solver keep across iterations
  auto store_iteration_scalars = [&](int next_phase) {
    if (sl == 0) {
      sc->f = f; sc->scaling_factor = scaling_factor; sc->xinf_bound = xinf_bound;
      sc->x_delta = x_delta; sc->f_delta = f_delta; sc->gradient_norm = gradient_norm;
      sc->mem_count = mem_count; sc->mem_pos = mem_pos; sc->status = status;
      sc->x_delta_violations = x_delta_violations; sc->f_delta_violations = f_delta_violations;
      sc->past_init = past_init; sc->past_pos = past_pos;
      sc->nfev = nfev; sc->sum_k = sum_k; sc->num_iterations = num_iterations;
      sc->phase = next_phase;
    }
  };

  bool need_update = false;     // s, y, the ring push, Progress::Update are due
  double xn[E], gn[E];          // the state the search returned
  double fn = 0.0;

  if (phase == kPhaseFirst) {
    // ---- Solver::Minimize prologue (solver.h:189-194): the caller's f, g are the evaluation at x0 ----------------
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const bool in = sl * E + e < n;
      x[e] = in ? a.x_eval[base + e] : 0.0;
      g[e] = in ? a.g[base + e] : 0.0;
    }
    f = a.f[slot];
    nfev = 1;                               // reset_solver of lbfgs_kernel.hpp: everything else is the initial value above
    xinf_bound = seg_amax<W, E>(x);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      x[e] = xs[e];
      g[e] = gs[e];
    }
    f = sc->f; scaling_factor = sc->scaling_factor; xinf_bound = sc->xinf_bound;
    x_delta = sc->x_delta; f_delta = sc->f_delta; gradient_norm = sc->gradient_norm;
    mem_count = sc->mem_count; mem_pos = sc->mem_pos; status = sc->status;
    x_delta_violations = sc->x_delta_violations; f_delta_violations = sc->f_delta_violations;
    past_init = sc->past_init != 0; past_pos = sc->past_pos;
    nfev = sc->nfev; sum_k = sc->sum_k; num_iterations = sc->num_iterations;
    for (int i = sl; i < m; i += W) rho_l[i] = sc->rho[i];
    segment_fence();
    if (phase == kPhaseTrial) {
      // ---- the cvsrch loop body after the evaluation (more_thuente.h:200-252) --------------------------------------
#pragma unroll
      for (int e = 0; e < E; ++e) {
        d[e] = ds[e];
        gn[e] = (sl * E + e < n) ? a.g[base + e] : 0.0;
      }
      fn = a.f[slot];
      mt.load(sc);
      if (mt.after_evaluation(fn, [&]() { nfev++; return -seg_dot<W, E, AR>(gn, d); }) == 0) {  // (g.s)
        ask_trial();
        return true;
      }
      // the search ended: the accepted point, re-formed from the accepted step (as mt_cvsrch ends)
#pragma unroll
      for (int e = 0; e < E; ++e) xn[e] = AR::nmadd(mt.stp, d[e], x[e]);
    } else {
      // ---- no evaluation wanted: the refused search left x, f, g untouched ------------------------------------------
#pragma unroll
      for (int e = 0; e < E; ++e) {
        xn[e] = x[e];
        gn[e] = g[e];
      }
      fn = f;
    }
    need_update = true;
  }

  if (need_update) {
    // ---- after the search (lbfgs_kernel.hpp: s, y, curvature test, history push, scaling) ----------------------------
    const double fprev = f;
    double sv[E], yv[E];
    double s_inf = 0.0;
    if (!__builtin_isfinite(fn)) {  // return current (lbfgs.h:239-241): x, f, g stay
#pragma unroll
      for (int e = 0; e < E; ++e) sv[e] = 0.0;
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        sv[e] = xn[e] - x[e];  // :248
        yv[e] = gn[e] - g[e];  // :249
        x[e] = xn[e];
        g[e] = gn[e];
      }
      f = fn;
      s_inf = seg_amax<W, E>(sv);
      const double sy = seg_dot<W, E, AR>(sv, yv);   // :265
      const double yy = seg_dot<W, E, AR>(yv, yv);   // :290
      // :266-267, with the bound shortcuts of lbfgs_kernel.hpp (the decision is the reference's either way)
      bool accept = false;
      if (sy > 0.0) {
        const double ss_bound = ((n_as_double * s_inf) * s_inf) * (1.0 + 1e-9);
        const double rhs_bound = ((4.0 * eps * eps) * ss_bound) * yy;
        if (rhs_bound >= 1e-290 && sy * sy > rhs_bound) {
          accept = true;
        } else {
          const double ss = seg_dot<W, E, AR>(sv, sv);
          const double rhs = ((4.0 * eps * eps) * ss) * yy;
          if (rhs >= 1e-290 && sy * sy > rhs) {
            accept = true;
          } else {
            const double sy_threshold = eps * __builtin_sqrt(ss) * __builtin_sqrt(yy);  // :266
            accept = sy > sy_threshold;
          }
        }
      }
      if (accept) {                              // :267-280
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
        const double rho_new = (__builtin_fabs(sy) < eps) ? 0.0 : 1.0 / sy;
        if (sl == 0) {
          rho_l[slot] = rho_new;
          sc->rho[slot] = rho_new;
        }
        segment_fence();
      }
      if (yy > eps) {                            // :289-298
        const double temp_scaling = sy / yy;
        if (__builtin_isfinite(temp_scaling) && __builtin_fabs(temp_scaling) <= 1e7) {
          scaling_factor = dmax(temp_scaling, eps);
        }
      }
    }
    // ---- Progress::Update (progress.h:188-317) --------------------------------------------------------------------------
    num_iterations++;
    f_delta = __builtin_fabs(f - fprev);
    x_delta = s_inf;
    gradient_norm = seg_amax<W, E>(g);
    xinf_bound = (xinf_bound + x_delta) * (1.0 + 4.0 * eps);
    status = progress_stop_tests<W, E>(a.stop, a.stop.num_iterations, a.stop.gradient_norm, num_iterations, f, fprev,
                                       x_delta, f_delta, gradient_norm, xinf_bound, x, x_delta_violations,
                                       f_delta_violations, sc->past_f, past_init, past_pos, sl);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      xs[e] = x[e];
      gs[e] = g[e];
    }
    if (status != MI355_STATUS_CONTINUE) {
      // finished: frozen from here on; the evaluation buffer holds the returned x
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (sl * E + e < n) a.x_eval[base + e] = x[e];
      store_iteration_scalars(kPhaseFinished);
      return false;
    }
  } else {
    // the first evaluation: x0 and its gradient become the state
#pragma unroll
    for (int e = 0; e < E; ++e) {
      xs[e] = x[e];
      gs[e] = g[e];
    }
  }

  // ======================= Lbfgs::OptimizationStep up to the search (lbfgs.h:89-232) =====================================
#pragma unroll
  for (int e = 0; e < E; ++e) d[e] = g[e];  // :145
  const int k = mem_count;
  sum_k += k;
  {
    const bool full = (mem_count >= m);
    auto prev_slot = [&](int slot) { return (slot == 0) ? m - 1 : slot - 1; };
    auto next_slot = [&](int slot) { return (slot + 1 == m) ? 0 : slot + 1; };
    // first loop, newest -> oldest (:157-171); rho = 0 marks a pair the reference skips (alpha = beta = 0)
    int slot = full ? prev_slot(mem_pos) : k - 1;
    for (int i = k - 1; i >= 0; --i) {
      double sv[E], yv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        sv[e] = Ss[static_cast<long long>(slot) * P + e];
        yv[e] = Ys[static_cast<long long>(slot) * P + e];
      }
      const double alpha = rho_l[slot] * seg_dot<W, E, AR>(sv, d);
      if (sl == 0) alpha_l[i] = alpha;
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = AR::nmadd(alpha, yv[e], d[e]);
      slot = prev_slot(slot);
    }
#pragma unroll
    for (int e = 0; e < E; ++e) d[e] = d[e] * scaling_factor;  // :181
    segment_fence();
    // second loop, oldest -> newest (:185-196)
    slot = full ? mem_pos : 0;
    for (int i = 0; i < k; ++i) {
      double sv[E], yv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        sv[e] = Ss[static_cast<long long>(slot) * P + e];
        yv[e] = Ys[static_cast<long long>(slot) * P + e];
      }
      const double beta = rho_l[slot] * seg_dot<W, E, AR>(yv, d);
      const double c = alpha_l[i] - beta;
#pragma unroll
      for (int e = 0; e < E; ++e) d[e] = AR::madd(sv[e], c, d[e]);
      slot = next_slot(slot);
    }
    segment_fence();  // (alpha_l is rewritten by the next problem of this segment)
  }
  const double descent_direction = -seg_dot<W, E, AR>(g, d);  // :199; also cvsrch's dginit = g.s with s = -d
  double dginit = descent_direction;
  double alpha_init = 1.0;                                  // :207-213
  if (mem_count == 0) {
    const double dn = __builtin_sqrt(seg_dot<W, E, AR>(d, d));
    alpha_init = (dn > eps) ? 1.0 / dn : 1.0;
  }
  // :214-224 with the ||x|| bound of lbfgs_kernel.hpp
  bool invalid_direction;
  if (__builtin_isfinite(descent_direction) &&
      descent_direction <= -eps * (eps * dmax(1.0, n_as_double * xinf_bound))) {
    invalid_direction = false;
  } else {
    const double relative_eps = eps * dmax(1.0, __builtin_sqrt(seg_dot<W, E, AR>(x, x)));  // :93-95
    invalid_direction = !__builtin_isfinite(descent_direction) || descent_direction > -eps * relative_eps;
  }
  if (invalid_direction) {
#pragma unroll
    for (int e = 0; e < E; ++e) d[e] = -g[e];
    mem_count = 0;
    mem_pos = 0;
    const double gg = seg_dot<W, E, AR>(g, g);
    const double gnorm = __builtin_sqrt(gg);
    alpha_init = (gnorm > eps) ? 1.0 / gnorm : 1.0;
    dginit = gg;  // s = -d = g: the search sees g.g >= 0 and returns at once (quirk Q1)
  }
#pragma unroll
  for (int e = 0; e < E; ++e) ds[e] = d[e];

  if (dginit >= 0.0) {  // more_thuente.h:152-156: no evaluation; the next call finishes this iteration
    store_iteration_scalars(kPhaseNoEval);
    return true;
  }
  // ---- the search starts (more_thuente.h:158-177) and asks for its first trial -----------------------------------------
  store_iteration_scalars(kPhaseTrial);
  mt.start(f, dginit, alpha_init);
  ask_trial();
  return true;
}

// static LDS of a step kernel, per segment: 1 / (s.y) per ring slot and the alpha of the running recursion
constexpr int kRhoLds = MI355_LBFGS_MAX_M, kAlphaLds = MI355_LBFGS_MAX_M + 1;
template <int W>
constexpr int step_lds_bytes() {
  return (kWave / W) * (kRhoLds + kAlphaLds) * static_cast<int>(sizeof(double));
}

// One step of every row a.B counts, and the tally of the problems still active after it.  Dense (kListed false): row
// r is problem r and a.B the batch.  Listed: row s of x_eval / f / g belongs to problem ids[s], ids ascending, a.B is
// the LENGTH OF THE LIST (nothing of a step is indexed by the batch size) and the grid is sized from it.  (Why the grid
// loop is spelled here and not in a function the three paths share: run_steps of lbfgsb_ask_tell_kernel.hpp.)
template <int W, int E, bool kListed>
__device__ __forceinline__ void run_steps(const Args a, const long long* ids) {
  constexpr int kSegs = kWave / W;
  __shared__ double rho_lds[kSegs][kRhoLds];
  __shared__ double alpha_lds[kSegs][kAlphaLds];
  static_assert(sizeof(rho_lds) + sizeof(alpha_lds) == step_lds_bytes<W>(), "what the launch reports");
  const int lane = threadIdx.x;
  const int seg = lane / W;
  const int sl = lane % W;
  unsigned long long active_count = 0;  // wavefront-uniform
  const long long stride = static_cast<long long>(gridDim.x) * kSegs;
  for (long long first = static_cast<long long>(blockIdx.x) * kSegs; first < a.B; first += stride) {
    const long long slot = first + seg;
    bool active = false;
    if (slot < a.B) active = step_problem<W, E>(a, kListed ? ids[slot] : slot, slot, sl, rho_lds[seg], alpha_lds[seg]);
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

// (the state initialisation and the result gather are ask_tell_kernel_common.hpp's)

}  // namespace ask_tell
}  // namespace mi355
