// lbfgs_ask_tell_kernel.hpp — Lbfgs<F, m, MoreThuente>::Minimize in reverse communication: the solver state of every
// problem lives in HBM between calls, one kernel call advances every problem up to its next objective evaluation, and
// the CALLER evaluates the batch of trial points (torch ops, autograd, its own kernels) and hands f, g back.
//
// Device counterpart of the same reference code as lbfgs_kernel.hpp (Solver::Minimize solver/solver.h:181-224,
// Lbfgs::OptimizationStep solver/lbfgs.h:89-303, MoreThuente::cvsrch linesearch/more_thuente.h:137-256,
// Progress::Update solver/progress.h:153-327), cut at the objective evaluation: the statements are those of
// lbfgs_kernel.hpp and mt_cvsrch (more_thuente_device.hpp) on the same operands in the same order, so a callback that
// evaluates with the library's own functor reproduces the persistent exact kernel bit for bit.
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
  // more_thuente.h:140-147
  constexpr double xtol = 1e-15, ftol = 1e-4, gtol = 0.9, stpmin = 1e-15, stpmax = 1e15, xtrapf = 4.0;
  constexpr int maxfev = 20;

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

  // the search's scalars (mt_cvsrch), segment-uniform
  double stx = 0.0, fx = 0.0, dgx = 0.0, sty = 0.0, fy = 0.0, dgy = 0.0, stp = 0.0;
  double width = 0.0, width1 = 0.0, finit = 0.0, dginit = 0.0, stmin = 0.0, stmax = 0.0;
  bool brackt = false, stage1 = true;
  int infoc = 1, ls_nfev = 0;
  // more_thuente.h:179-195: the interval, the clamp and the fallback before an evaluation
  auto before_evaluation = [&]() {
    if (brackt) {
      stmin = dmin(stx, sty);
      stmax = dmax(stx, sty);
    } else {
      stmin = stx;
      stmax = stp + xtrapf * (stp - stx);
    }
    stp = dclamp(stp, stpmin, stpmax);
    if ((brackt && ((stp <= stmin) || (stp >= stmax))) || (ls_nfev >= maxfev - 1) || (infoc == 0) ||
        (brackt && ((stmax - stmin) <= (xtol * stmax)))) {
      stp = stx;
    }
  };
  // the trial point wa + stp s = x - stp d into the evaluation buffer, and the search's scalars
  auto ask_trial = [&]() {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (sl * E + e < n) a.x_eval[base + e] = AR::nmadd(stp, d[e], x[e]);
    if (sl == 0) {
      sc->stx = stx; sc->fx = fx; sc->dgx = dgx;
      sc->sty = sty; sc->fy = fy; sc->dgy = dgy;
      sc->stp = stp; sc->width = width; sc->width1 = width1;
      sc->finit = finit; sc->dginit = dginit; sc->stmin = stmin; sc->stmax = stmax;
      sc->brackt = brackt; sc->stage1 = stage1; sc->infoc = infoc; sc->ls_nfev = ls_nfev;
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
      stx = sc->stx; fx = sc->fx; dgx = sc->dgx;
      sty = sc->sty; fy = sc->fy; dgy = sc->dgy;
      stp = sc->stp; width = sc->width; width1 = sc->width1;
      finit = sc->finit; dginit = sc->dginit; stmin = sc->stmin; stmax = sc->stmax;
      brackt = sc->brackt != 0; stage1 = sc->stage1 != 0; infoc = sc->infoc; ls_nfev = sc->ls_nfev;
      const double dgtest = ftol * dginit;
      ls_nfev++;
      nfev++;
      const double dg = -seg_dot<W, E, AR>(gn, d);  // g.s
      const double ftest1 = finit + stp * dgtest;
      int info = 0;
      if ((brackt & ((stp <= stmin) | (stp >= stmax))) | (infoc == 0)) info = 6;
      if ((stp == stpmax) & (fn <= ftest1) & (dg <= dgtest)) info = 5;
      if ((stp == stpmin) & ((fn > ftest1) | (dg >= dgtest))) info = 4;
      if (ls_nfev >= maxfev) info = 3;
      if (brackt & (stmax - stmin <= xtol * stmax)) info = 2;
      if ((fn <= ftest1) & (__builtin_fabs(dg) <= gtol * (-dginit))) info = 1;
      if (info == 0) {
        if (stage1 & (fn <= ftest1) & (dg >= dmin(ftol, gtol) * dginit)) stage1 = false;
        const bool modified = stage1 & (fn <= fx) & (fn > ftest1);
        StepInterval iv;
        iv.stx = stx; iv.sty = sty; iv.stp = stp; iv.brackt = brackt; iv.info = infoc; iv.rc = 0;
        iv.fx = modified ? fx - stx * dgtest : fx;
        iv.fy = modified ? fy - sty * dgtest : fy;
        iv.dx = modified ? dgx - dgtest : dgx;
        iv.dy = modified ? dgy - dgtest : dgy;
        const double fm = modified ? fn - stp * dgtest : fn;
        const double dgm = modified ? dg - dgtest : dg;
        iv = mt_cstep(iv, fm, dgm, stmin, stmax);
        stx = iv.stx; sty = iv.sty; stp = iv.stp; brackt = iv.brackt; infoc = iv.info;
        fx = modified ? iv.fx + stx * dgtest : iv.fx;
        fy = modified ? iv.fy + sty * dgtest : iv.fy;
        dgx = modified ? iv.dx + dgtest : iv.dx;
        dgy = modified ? iv.dy + dgtest : iv.dy;
        if (brackt) {
          if (__builtin_fabs(sty - stx) >= 0.66 * width1) stp = stx + 0.5 * (sty - stx);
          width1 = width;
          width = __builtin_fabs(sty - stx);
        }
        before_evaluation();
        ask_trial();
        return true;
      }
      // the search ended: the accepted point, re-formed from the accepted step (more_thuente_device.hpp:413)
#pragma unroll
      for (int e = 0; e < E; ++e) xn[e] = AR::nmadd(stp, d[e], x[e]);
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
  dginit = descent_direction;
  double alpha_init = 1.0;                                    // :207-213
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
  brackt = false;
  stage1 = true;
  infoc = 1;
  ls_nfev = 0;
  finit = f;
  width = stpmax - stpmin;
  width1 = 2.0 * width;
  stx = 0.0; fx = finit; dgx = dginit;
  sty = 0.0; fy = finit; dgy = dginit;
  stp = alpha_init;
  before_evaluation();
  ask_trial();
  return true;
}

template <int W, int E>
__global__ __launch_bounds__(64) void step_kernel(const Args a) {
  constexpr int kSegs = kWave / W;
  __shared__ double rho_lds[kSegs][MI355_LBFGS_MAX_M];
  __shared__ double alpha_lds[kSegs][MI355_LBFGS_MAX_M + 1];
  const int lane = threadIdx.x;
  const int seg = lane / W;
  const int sl = lane % W;
  unsigned long long active_count = 0;  // wavefront-uniform
  const long long stride = static_cast<long long>(gridDim.x) * kSegs;
  for (long long first = static_cast<long long>(blockIdx.x) * kSegs; first < a.B; first += stride) {
    const long long prob = first + seg;
    bool active = false;
    if (prob < a.B) active = step_problem<W, E>(a, prob, prob, sl, rho_lds[seg], alpha_lds[seg]);
    active_count += __builtin_popcountll(__builtin_amdgcn_ballot_w64(active && sl == 0));
  }
  if (lane == 0 && active_count != 0) atomicAdd(a.active, active_count);
}

// The same step on a compacted handle (a kernel of its own: step_kernel stays as it was built before there were lists):
// slot s of x_eval / f / g belongs to problem ids[s], ids ascending.  a.B is the LENGTH OF THE LIST here (nothing of a
// step is indexed by the batch size), and the grid is sized from it.
template <int W, int E>
__global__ __launch_bounds__(64) void listed_step_kernel(const Args a, const long long* ids) {
  constexpr int kSegs = kWave / W;
  __shared__ double rho_lds[kSegs][MI355_LBFGS_MAX_M];
  __shared__ double alpha_lds[kSegs][MI355_LBFGS_MAX_M + 1];
  const int lane = threadIdx.x;
  const int seg = lane / W;
  const int sl = lane % W;
  unsigned long long active_count = 0;  // wavefront-uniform
  const long long stride = static_cast<long long>(gridDim.x) * kSegs;
  for (long long first = static_cast<long long>(blockIdx.x) * kSegs; first < a.B; first += stride) {
    const long long slot = first + seg;
    bool active = false;
    if (slot < a.B) active = step_problem<W, E>(a, ids[slot], slot, sl, rho_lds[seg], alpha_lds[seg]);
    active_count += __builtin_popcountll(__builtin_amdgcn_ballot_w64(active && sl == 0));
  }
  if (lane == 0 && active_count != 0) atomicAdd(a.active, active_count);
}

// (the state initialisation and the result gather are ask_tell_kernel_common.hpp's)

}  // namespace ask_tell
}  // namespace mi355
