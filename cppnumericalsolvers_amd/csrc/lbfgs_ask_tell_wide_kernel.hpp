// lbfgs_ask_tell_wide_kernel.hpp — Lbfgs<F, m, MoreThuente>::Minimize in reverse communication for problems LARGER than a
// wavefront segment holds (n > 256): the solver state of every problem lives in HBM between calls, one kernel call
// advances every problem up to its next objective evaluation, and the CALLER evaluates the batch of trial points.
//
// The two halves it joins: the mapping, the sums and the statements are those of
// lbfgs_wide_kernel<Obj, 0, MI355_LS_MORE_THUENTE, T> (lbfgs_wide_kernel.hpp) on the same operands in the same order —
// no xinf / ss bound shortcuts, x . x, max |g_j| and max |x_j| carried with the iterate, pairs with |s . y| < eps skipped,
// every element-wise update of the two-loop recursion fused with the inner product that follows it, g . d at the trial
// point from the gradient's own pass, the last evaluated trial taken as `next` — cut at obj.eval; the phase machine, the
// bounded-work rule and the resumable search (MtSearch<double>) are those of lbfgs_ask_tell_kernel.hpp.  A callback
// that evaluates with the library's own workgroup functor (mi355_lbfgs_eval_batch above n = 256) therefore reproduces
// the persistent wide kernel bit for bit.
//
// Mapping: one problem per workgroup of T threads (256, or 1024 for n >= kWideBigN: a function of n alone, and so is the
// summation order); thread t owns the coordinates j = t, t + T, ... in ascending order (coalesced: lane t of a wavefront
// reads element t + T e); every sum is wide_sum / wide_reduce.  The grid strides over the rows of the call; there is no
// work queue.  Scalars are read by every thread (one address per workgroup) and written by thread 0.
//
// State row of a problem (np = n rounded up to even): x | g | d | S[m] | Y[m]; the trial point lives in x_eval.  While
// the launch carries np doubles of dynamic LDS (n <= 4096, as launch_wide decides) the direction sits there during the
// recursion and reaches its row with the first trial point: same operations, same bits.
//
// One call does a bounded amount of work per problem, in this order:
//   1. trial pending: the gradient's pass for g . d, MtSearch::load / after_evaluation / store; info == 0: the next
//      trial point into x_eval, return
//   2. search ended / no evaluation wanted: the fused 4-sum / 3-max pass over s and y, ring push, gamma,
//      Progress::Update and the stopping tests
//   3. going on (also after the first evaluation): two-loop recursion over <= m slots, descent test with fallback,
//      alpha_init
//   4. the first trial point of the next search into x_eval — or, where that search is refused at once (dginit >= 0),
//      the phase "no evaluation wanted".
#pragma once
#include "lbfgs_ask_tell_wide_config.hpp"
#include "lbfgs_wide_kernel.hpp"

namespace mi355 {
namespace ask_tell_wide {

// static LDS of a step kernel: the reduction scratch, s . y by ring slot, alpha by chronological index, the plateau ring
struct StepLds {
  double red[8 * kWideMaxWaves];
  double sy_mem[kWideMaxM];
  double alpha_mem[kWideMaxM];
  double past_f[MI355_LBFGS_MAX_PAST];
};

// body(j) for every coordinate j = tid + T e < n of the calling thread, ascending
template <class F>
__device__ __forceinline__ void for_own(int n, F&& body) {
  for (int j = threadIdx.x; j < n; j += wide_threads()) body(j);
}

// One step of problem `prob` on the calling workgroup.  `slot`: its row of the caller's arrays (x_eval, f, g) — `prob`
// itself, or its place in the list of a compacted handle; everything else is indexed by `prob`.  d_lds: np doubles of
// LDS, or nullptr.  Returns (to every thread) whether the problem is still active after the call.
__device__ __forceinline__ bool step_problem(const Args& a, long long prob, long long slot, StepLds& lds, double* d_lds) {
  constexpr double eps = 2.220446049250313e-16;
  Scalars* const sc = a.scalars + prob;
  const int phase = sc->phase;
  if (phase == kPhaseFinished) return false;

  const int tid = threadIdx.x;
  const int n = a.n, m = a.m;
  const long long np = padded(n);
  double* const row = a.vectors + prob * row_doubles(m, np);
  double* const x = row;
  double* const g = row + np;
  double* const ds = row + 2 * np;
  double* const S = row + 3 * np;
  double* const Y = S + static_cast<long long>(m) * np;
  double* const xe = a.x_eval + slot * n;  // of the caller's [rows][n] arrays
  const double* const gin = a.g + slot * n;
  double* const red = lds.red;
  double* const sy_mem = lds.sy_mem;
  double* const alpha_mem = lds.alpha_mem;
  double* const past_f = lds.past_f;

  double f = 0.0, scaling_factor = 1.0, xx_cur = 0.0, gmax_cur = 0.0, xmax_cur = 0.0;
  double x_delta = 0.0, f_delta = 0.0, gradient_norm = 0.0;
  int mem_count = 0, mem_pos = 0, status = MI355_STATUS_NOT_STARTED, x_delta_violations = 0, f_delta_violations = 0;
  int past_pos = 0;
  bool past_init = false;
  unsigned nfev = 0, sum_k = 0, num_iterations = 0;
  MtSearch<double> mt;  // the running search, workgroup-uniform

  // what Progress and the solver keep across iterations
  auto store_iteration_scalars = [&](int next_phase) {
    if (tid == 0) {
      sc->f = f; sc->scaling_factor = scaling_factor;
      sc->xx_cur = xx_cur; sc->gmax_cur = gmax_cur; sc->xmax_cur = xmax_cur;
      sc->x_delta = x_delta; sc->f_delta = f_delta; sc->gradient_norm = gradient_norm;
      sc->mem_count = mem_count; sc->mem_pos = mem_pos; sc->status = status;
      sc->x_delta_violations = x_delta_violations; sc->f_delta_violations = f_delta_violations;
      sc->past_init = past_init; sc->past_pos = past_pos;
      sc->nfev = nfev; sc->sum_k = sum_k; sc->num_iterations = num_iterations;
      sc->phase = next_phase;
    }
  };

  bool need_update = false;      // s, y, the ring push, Progress::Update are due
  const double* xn = x;          // next.x and next.gradient: the state the search returned
  const double* gn = g;
  double f_next = 0.0;

  if (phase == kPhaseFirst) {
    // ---- Solver::Minimize prologue (solver.h:189-194): the caller's f, g are the evaluation at x0 ----------------
    // with x . x, max |g_j| and max |x_j| of the start (lbfgs_wide_kernel: carried with the current iterate)
    double sums[1] = {0.0}, maxs[2] = {0.0, 0.0};
    for_own(n, [&](int j) {
      const double xj = xe[j], gj = gin[j];
      x[j] = xj;
      g[j] = gj;
      sums[0] = sums[0] + xj * xj;
      const double ta = __builtin_fabs(gj), tb = __builtin_fabs(xj);
      if (maxs[0] < ta) maxs[0] = ta;
      if (maxs[1] < tb) maxs[1] = tb;
    });
    wide_reduce<1, 2>(sums, maxs, red);
    xx_cur = sums[0];
    gmax_cur = maxs[0];
    xmax_cur = maxs[1];
    f = a.f[slot];
    nfev = 1;  // everything else is the initial value above
  } else {
    f = sc->f; scaling_factor = sc->scaling_factor;
    xx_cur = sc->xx_cur; gmax_cur = sc->gmax_cur; xmax_cur = sc->xmax_cur;
    x_delta = sc->x_delta; f_delta = sc->f_delta; gradient_norm = sc->gradient_norm;
    mem_count = sc->mem_count; mem_pos = sc->mem_pos; status = sc->status;
    x_delta_violations = sc->x_delta_violations; f_delta_violations = sc->f_delta_violations;
    past_init = sc->past_init != 0; past_pos = sc->past_pos;
    nfev = sc->nfev; sum_k = sc->sum_k; num_iterations = sc->num_iterations;
    if (phase == kPhaseTrial) mt.load(sc);
    __syncthreads();  // the previous row's readers are done with the LDS scalars
    if (tid < m) sy_mem[tid] = sc->sy[tid];
    if (tid < MI355_LBFGS_MAX_PAST) past_f[tid] = sc->past_f[tid];
    __syncthreads();  // ... and every thread has read the scalars thread 0 rewrites below
    if (phase == kPhaseTrial) {
      // ---- the cvsrch loop body after the evaluation (more_thuente.h:200-252); g . d from the gradient's own pass ----
      double acc = 0.0;
      for_own(n, [&](int j) { acc = acc + gin[j] * ds[j]; });
      const double gdn = wide_sum(acc, red);
      f_next = a.f[slot];
      nfev++;
      if (mt.after_evaluation(f_next, [&] { return -gdn; }) == 0) {  // (g . s)
        const double stp = mt.stp;
        for_own(n, [&](int j) { xe[j] = stp * (-ds[j]) + x[j]; });  // wa + stp * s
        if (tid == 0) {
          mt.store(sc);
          sc->nfev = nfev;
        }
        return true;
      }
      // the search ended: next is the last evaluated trial, as the caller holds it
      xn = xe;
      gn = gin;
    } else {
      // ---- no evaluation wanted: the refused search left next = current -------------------------------------------
      f_next = f;
    }
    need_update = true;
  }

  if (need_update) {
    // ---- lbfgs.h:239-298 and the norms of Progress::Update (progress.h:188-195), one pass ---------------------------
    const double f_prev = f;
    if (__builtin_isfinite(f_next)) {
      double sums[4] = {0.0, 0.0, 0.0, 0.0};   // s.y, s.s, y.y, next.x . next.x
      double maxs[3] = {0.0, 0.0, 0.0};        // max |s_j| (x_delta), max |next.g_j|, max |next.x_j|
      for_own(n, [&](int j) {
        const double xj = xn[j], gj = gn[j];
        const double sj = xj - x[j], yj = gj - g[j];
        sums[0] = sums[0] + sj * yj;
        sums[1] = sums[1] + sj * sj;
        sums[2] = sums[2] + yj * yj;
        sums[3] = sums[3] + xj * xj;
        const double ta = __builtin_fabs(sj), tb = __builtin_fabs(gj), tc = __builtin_fabs(xj);
        if (maxs[0] < ta) maxs[0] = ta;
        if (maxs[1] < tb) maxs[1] = tb;
        if (maxs[2] < tc) maxs[2] = tc;
      });
      wide_reduce<4, 3>(sums, maxs, red);
      const double sy = sums[0], ss = sums[1], yy = sums[2];
      const double sy_threshold = eps * __builtin_sqrt(ss) * __builtin_sqrt(yy);          // :266
      const bool push = sy > sy_threshold;                                                 // :267-280
      if (push) {
        const int ring = (mem_count < m) ? mem_count : mem_pos;
        double* const s = S + static_cast<long long>(ring) * np;
        double* const y = Y + static_cast<long long>(ring) * np;
        // the pair into the ring, and next becomes current (a thread's own coordinates: no barrier)
        for_own(n, [&](int j) {
          const double xj = xn[j], gj = gn[j];
          s[j] = xj - x[j];
          y[j] = gj - g[j];
          x[j] = xj;
          g[j] = gj;
        });
        if (tid == 0) {
          sy_mem[ring] = sy;
          sc->sy[ring] = sy;
        }
        if (mem_count < m) {
          mem_count++;
        } else {
          mem_pos = (mem_pos + 1) % m;
        }
      } else if (xn != x) {
        for_own(n, [&](int j) {
          x[j] = xn[j];
          g[j] = gn[j];
        });
      }
      constexpr double fallback_value = 1e7;                                              // :289-298
      if (yy > eps) {
        const double temp_scaling = sy / yy;   // y.dot(s): the same products as s.dot(y)
        if (__builtin_isfinite(temp_scaling) && __builtin_fabs(temp_scaling) <= fallback_value)
          scaling_factor = dmax(temp_scaling, eps);
      }
      f = f_next;
      x_delta = maxs[0];
      xx_cur = sums[3];
      gmax_cur = maxs[1];
      xmax_cur = maxs[2];
    } else {
      x_delta = 0.0;   // :239-241: the step returns `current`, so previous == current for the tests below
    }

    // ================= Progress::Update, progress.h:153-327 (lbfgs_wide_kernel's tests) ==========================
    num_iterations++;
    f_delta = __builtin_fabs(f - f_prev);
    gradient_norm = gmax_cur;
    status = MI355_STATUS_CONTINUE;
    const mi355_lbfgs_stop& st = a.stop;
    do {
      if ((st.num_iterations > 0) && (num_iterations > st.num_iterations)) {              // :212-216
        status = MI355_STATUS_ITERATION_LIMIT;
        break;
      }
      if ((st.x_delta > 0) && (x_delta < st.x_delta)) {                                    // :254-262
        x_delta_violations++;
        if (x_delta_violations >= st.x_delta_violations) {
          status = MI355_STATUS_X_DELTA_VIOLATION;
          break;
        }
      } else {
        x_delta_violations = 0;
      }
      if ((st.f_delta > 0) &&                                                              // :263-277
          (f_delta < st.f_delta * (st.f_delta_relative
                                       ? dmax(dmax(__builtin_fabs(f), __builtin_fabs(f_prev)), 1.0)
                                       : 1.0))) {
        f_delta_violations++;
        if (f_delta_violations >= st.f_delta_violations) {
          status = MI355_STATUS_F_DELTA_VIOLATION;
          break;
        }
      } else {
        f_delta_violations = 0;
      }
      if (st.past > 0) {                                                                   // :280-298
        const int p = st.past;
        __syncthreads();
        if (!past_init) {
          if (tid < p) {
            past_f[tid] = f;
            sc->past_f[tid] = f;
          }
          past_init = true;
          past_pos = 0;
        }
        __syncthreads();
        bool fired = false;
        if (num_iterations > static_cast<unsigned>(p)) {
          const double pf = past_f[past_pos];
          const double rate = __builtin_fabs(pf - f) / dmax(1.0, __builtin_fabs(f));
          fired = rate < st.past_delta;
        }
        if (fired) {
          status = MI355_STATUS_F_DELTA_VIOLATION;
          break;
        }
        __syncthreads();
        if (tid == 0) {
          past_f[past_pos] = f;
          sc->past_f[past_pos] = f;
        }
        past_pos = (past_pos + 1) % p;
      }
      if (st.gradient_norm > 0) {                                                          // :299-317
        const double scale = st.gradient_norm_relative ? dmax(1.0, xmax_cur) : 1.0;
        if (gradient_norm < st.gradient_norm * scale) {
          status = MI355_STATUS_GRADIENT_NORM_VIOLATION;
          break;
        }
      }
    } while (false);
    if (status != MI355_STATUS_CONTINUE) {
      // finished: frozen from here on; the evaluation buffer holds the returned x
      for_own(n, [&](int j) { xe[j] = x[j]; });
      store_iteration_scalars(kPhaseFinished);
      return false;
    }
  }

  // ================= Lbfgs::OptimizationStep up to the search, lbfgs.h:89-232 ===========================================
  __syncthreads();  // sy_mem of the pair stored above (written by thread 0)
  double* const d = d_lds ? d_lds : ds;
  const double relative_eps = eps * dmax(1.0, __builtin_sqrt(xx_cur));                   // :93-95
  const int k = mem_count;
  sum_k += static_cast<unsigned>(k);
  // The two-loop recursion :145-196 with every element-wise update fused with the inner product that follows it:
  // one sweep per step.  Pairs with |s.y| < eps are skipped (:165, :189).
  auto slot_of = [&](int i) { return (mem_count < m) ? i : ((mem_pos + i) % m); };
  auto active = [&](int i) { return !(__builtin_fabs(sy_mem[slot_of(i)]) < eps); };
  auto next_down = [&](int i) { do { --i; } while (i >= 0 && !active(i)); return i; };
  auto next_up = [&](int i) { do { ++i; } while (i < k && !active(i)); return i; };
  const int first = next_up(-1);   // oldest active pair (k: none)
  double gd, dd = 0.0;
  if (first >= k) {
    // no usable pair: d = g * scaling_factor_, with g.d and (for alpha_init) d.d on the way
    double sums[2] = {0.0, 0.0}, none[1] = {0.0};
    for_own(n, [&](int j) {
      const double gj = g[j];
      const double dj = scaling_factor * gj;
      d[j] = dj;
      sums[0] = sums[0] + gj * dj;
      sums[1] = sums[1] + dj * dj;
    });
    wide_reduce<2, 0>(sums, none, red);
    gd = sums[0];
    dd = sums[1];
  } else {
    // first loop, newest -> oldest
    int i = next_down(k);
    double acc = 0.0;
    {
      const double* const s = S + static_cast<long long>(slot_of(i)) * np;
      for_own(n, [&](int j) {
        const double gj = g[j];
        d[j] = gj;                                                                       // :145
        acc = acc + s[j] * gj;
      });
    }
    while (true) {
      const int idx = slot_of(i);
      const double alpha = (1.0 / sy_mem[idx]) * wide_sum(acc, red);                     // rho * s.d
      if (tid == 0) alpha_mem[i] = alpha;
      const double* const y = Y + static_cast<long long>(idx) * np;
      const int inext = next_down(i);
      acc = 0.0;
      if (inext >= 0) {
        const double* const s = S + static_cast<long long>(slot_of(inext)) * np;
        for_own(n, [&](int j) {
          const double dj = d[j] - alpha * y[j];
          d[j] = dj;
          acc = acc + s[j] * dj;
        });
        i = inext;
      } else {
        // last step of the first loop: the scaling (:181) and the second loop's first inner product ride along
        const double* const y0 = Y + static_cast<long long>(slot_of(first)) * np;
        for_own(n, [&](int j) {
          const double dj = scaling_factor * (d[j] - alpha * y[j]);
          d[j] = dj;
          acc = acc + y0[j] * dj;
        });
        break;
      }
    }
    // second loop, oldest -> newest (:185-196)
    i = first;
    while (true) {
      const int idx = slot_of(i);
      const double beta = (1.0 / sy_mem[idx]) * wide_sum(acc, red);                      // rho * y.d
      const double c = alpha_mem[i] - beta;   // (written by thread 0 before at least one barrier pair)
      const double* const s = S + static_cast<long long>(idx) * np;
      const int inext = next_up(i);
      acc = 0.0;
      if (inext < k) {
        const double* const y = Y + static_cast<long long>(slot_of(inext)) * np;
        for_own(n, [&](int j) {
          const double dj = s[j] * c + d[j];
          d[j] = dj;
          acc = acc + y[j] * dj;
        });
        i = inext;
      } else {
        for_own(n, [&](int j) {
          const double dj = s[j] * c + d[j];
          d[j] = dj;
          acc = acc + g[j] * dj;
        });
        gd = wide_sum(acc, red);
        break;
      }
    }
  }
  const double descent_direction = -gd;                                                  // :199
  double alpha_init = 1.0;                                                               // :207-213
  if (mem_count == 0) {
    const double dn = __builtin_sqrt(dd);
    alpha_init = (dn > eps) ? 1.0 / dn : 1.0;
  }
  double dginit = descent_direction;  // g . (-d), bit for bit
  if (!__builtin_isfinite(descent_direction) || descent_direction > -eps * relative_eps) {  // :214-224
    double gg = 0.0;
    for_own(n, [&](int j) {
      const double gj = g[j];
      d[j] = -gj;
      gg = gg + gj * gj;
    });
    gg = wide_sum(gg, red);
    mem_count = 0;
    mem_pos = 0;
    const double gnorm = __builtin_sqrt(gg);
    alpha_init = (gnorm > eps) ? 1.0 / gnorm : 1.0;
    dginit = gg;  // g . (-d) = g . g: the products are the same, so is the sum
  }

  if (dginit >= 0.0) {  // more_thuente.h:152-156: no evaluation; the next call finishes this iteration
    store_iteration_scalars(kPhaseNoEval);
    return true;
  }
  // ---- the search starts (more_thuente.h:158-177) and asks for its first trial; the direction into its row -----------
  mt.start(f, dginit, alpha_init);
  {
    const double stp = mt.stp;
    for_own(n, [&](int j) {
      const double dj = d[j];
      if (d_lds) ds[j] = dj;
      xe[j] = stp * (-dj) + x[j];  // wa + stp * s
    });
  }
  store_iteration_scalars(kPhaseTrial);
  if (tid == 0) mt.store(sc);
  return true;
}

// One step of every row a.B counts, and the tally of the problems still active after it.  Dense (kListed false): row
// r is problem r and a.B the batch.  Listed: row s of x_eval / f / g belongs to problem ids[s], ids ascending, a.B is
// the LENGTH OF THE LIST and the grid is sized from it.  A workgroup strides over the rows.
template <int T, bool kListed>
__device__ __forceinline__ void run_steps(const Args& a, const long long* ids) {
  __shared__ StepLds lds;
  extern __shared__ double atw_direction_lds[];
  double* const d_lds = a.d_in_lds ? atw_direction_lds : nullptr;
  unsigned long long active_count = 0;  // workgroup-uniform
  for (long long slot = blockIdx.x; slot < a.B; slot += gridDim.x)
    active_count += step_problem(a, kListed ? ids[slot] : slot, slot, lds, d_lds) ? 1ULL : 0ULL;
  if (threadIdx.x == 0 && active_count != 0) atomicAdd(a.active, active_count);
}

// The two entry points of run_steps: two kernels, so that the dense one takes no list argument and tests none.
template <int T>
__global__ __launch_bounds__(T) void step_kernel(const Args a) {
  run_steps<T, false>(a, nullptr);
}

template <int T>
__global__ __launch_bounds__(T) void listed_step_kernel(const Args a, const long long* ids) {
  run_steps<T, true>(a, ids);
}

// One objective evaluation per row with the workgroup functor of the persistent wide kernel (mi355_lbfgs_eval_batch above
// n = 256): a workgroup strides over the rows; g_out[row] receives the gradient, f_out[row] the value.
template <class Obj, int T>
__global__ __launch_bounds__(T) void eval_kernel(const double* x, double* f_out, double* g_out, const double* obj_params,
                                                 long long B, int n) {
  __shared__ double red[8 * kWideMaxWaves];
  Obj obj;
  obj.load(obj_params, n);
  for (long long r = blockIdx.x; r < B; r += gridDim.x) {
    WideVec<0> xv, gv;
    xv.mem = const_cast<double*>(x) + r * n;
    gv.mem = g_out + r * n;
    const double f = obj.template eval<0>(xv, gv, n, red, nullptr);
    if (threadIdx.x == 0) f_out[r] = f;
  }
}

}  // namespace ask_tell_wide
}  // namespace mi355
