// nelder_mead_kernel.hpp — the whole NelderMead solve of one problem on one wavefront segment.
//
// Device counterpart of
//   Solver::Minimize               solver/solver.h:181-224        (driver loop, the state rebuild of :210-216)
//   NelderMead::OptimizationStep   solver/nelder_mead.h:102-195   (ordering, restart, centroid, the moves)
//   makeInitialSimplex             :202-217
//   isCoincident, shrink           :220-234
//   Progress::Update               solver/progress.h:153-327      (solver_driver.hpp, progress_device.hpp)
//
// Mapping.  A problem of dimension n <= W is owned by a segment of W consecutive lanes, one coordinate per lane (E = 1):
// lane j keeps coordinate j of the returned iterate, of the centroid and of the trial points in registers.  In the
// segment's LDS: the simplex, n x (n + 1) column major (lane j reads and writes row j: consecutive doubles across
// lanes), the n + 1 vertex values, and the rank permutation idx (idx[r] = the vertex of rank r).
//   ordering   vertex v gets rank #{u : f_u < f_v, or f_u and f_v unordered-or-equal and u < v}: the order of the
//              reference's comparator `f[a] < f[b]` with ties broken by the lower vertex index (a NaN ranks after every
//              number, so the ranks are a permutation whatever the values).  Lane sl counts for the vertices sl, sl + W.
//   centroid   lane j adds its coordinate of the n best vertices in rank order and divides by n: element-wise, the
//              reference's order exactly.  Every move is element-wise too, with the reference's grouping of products.
//   f(v)       the functor's value<W, 1> on the segment (its butterfly sum); every scalar of the algorithm is a vertex
//              value or a segment reduction, so control flow is uniform over a segment.
//
// Cached values.  The reference re-evaluates all n + 1 vertices at the start of every step (:111-114).  The objective is a
// pure function, so a vertex that has not moved has the value it had: the values stay in LDS and only new points are
// evaluated (one or two per ordinary step, n on a shrink).  progress.nfev still counts what the reference calls — n + 1
// per step, n + 1 on a restart, 1 for the reflection, 1 for an expansion or contraction, n + 1 on a shrink (the best
// vertex included, :229-233), 1 for the state rebuild, 1 for the initial state — which is the move of the trust-region
// kernel's counted retries (trust_region_kernel.hpp): what a repeated call would return is known, so it is counted,
// not run.
//
// Returned iterate.  The step returns simplex.col(idx[0]) with idx as sorted at the start of the step (after a restart:
// of the restarted simplex): when the reflected or expanded point beats the best vertex the step still returns the old
// best vertex (:194).  Reproduced.
//
// Modes.  FIRST = false is DifferentiabilityMode::None: no gradient is formed, gradient_norm stays 0 and the gradient
// test is off.  FIRST = true is the reference on a First-mode functor: the state rebuild evaluates value and gradient
// at the returned vertex once per step (the functor's eval), and Progress::Update's gradient test applies.
// Exact arithmetic only (-ffp-contract=off).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/mi355_lbfgs.h"
#include "lbfgs_kernel.hpp"
#include "nelder_mead_config.hpp"
#include "objectives.hpp"
#include "solver_driver.hpp"
#include "wave_primitives.hpp"

namespace mi355 {

// LDS doubles one problem needs: the simplex, the vertex values and the rank permutation (one double-sized slot each)
__host__ __device__ inline int nelder_mead_lds_doubles(int n, int /*W*/) { return n * (n + 1) + 2 * (n + 1); }

// functors with a value-and-gradient entry (eval) can run in first mode; value-only user functors define value alone
template <class Obj, class = void>
struct HasGradientEval : std::false_type {};
template <class Obj>
struct HasGradientEval<Obj, std::void_t<decltype(&Obj::template eval<8, 1>)>> : std::true_type {};

template <int W, class Obj, bool FIRST>
__global__ __launch_bounds__(64) void nelder_mead_kernel(const SolveArgs a, const NelderMeadDeviceConfig cfg) {
  static_assert(Obj::kLdsDoubles == 0 && Obj::shared_lds_doubles() == 0,
                "the Nelder-Mead kernel is built for functors without LDS data");
  extern __shared__ __attribute__((aligned(16))) double lds[];

  const int lane = threadIdx.x & (kWave - 1);
  const int seg = lane / W;
  const int sl = lane % W;
  const int n = a.n;
  const int nv = n + 1;
  const bool own = sl < n;
  const long long queue_length = queue_length_of(a);
  double* const S = lds + seg * nelder_mead_lds_doubles(n, W);
  double* const fv = S + n * nv;
  int* const idx = reinterpret_cast<int*>(fv + nv);
  double* const past_f = plateau_ring_slot<W>(a, seg);
  const double stop_gradient_norm = FIRST ? a.stop.gradient_norm : 0.0;

  Obj obj;
  obj.load(a.obj_params, n, sl, nullptr, nullptr);

  auto value_of = [&](double xj) -> double {
    double xv[1] = {own ? xj : 0.0};
    return obj.template value<W, 1>(xv, n, sl);
  };
  // the value of vertex v into the cache
  auto evaluate_vertex = [&](int v) {
    const double fval = value_of(own ? S[sl + v * n] : 0.0);
    if (sl == 0) fv[v] = fval;
  };
  // makeInitialSimplex (:202-217) around the point whose coordinate this lane holds, and the values of its vertices
  auto make_simplex = [&](double xj) {
    segment_lds_fence();
    if (own) {
      const double ax = __builtin_fabs(xj);
      const double delta = (ax > 1e-6) ? 0.05 * ax : 0.001;
      for (int c = 0; c < nv; ++c) S[sl + c * n] = (sl == c - 1) ? xj + delta : xj;
    }
    segment_lds_fence();
    for (int v = 0; v < nv; ++v) evaluate_vertex(v);
    segment_lds_fence();
  };
  // idx <- the vertices by value, ties by the lower index (std::sort's comparator :117-118 made a total order)
  auto rank_vertices = [&]() {
    for (int v = sl; v < nv; v += W) {
      const double fvv = fv[v];
      const bool v_nan = fvv != fvv;
      int r = 0;
      for (int u = 0; u < nv; ++u) {
        const double fu = fv[u];
        const bool u_nan = fu != fu;
        const bool u_less = (fu < fvv) || (v_nan && !u_nan);
        const bool v_less = (fvv < fu) || (u_nan && !v_nan);
        r += (u_less || (!v_less && u < v)) ? 1 : 0;
      }
      idx[r] = v;
    }
    segment_lds_fence();
  };

  double x[1], g[1] = {0.0};
  double f = 0.0;
  SolveProgress prog;                                      // prog.sum_k stays 0: this solver has no inner count
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
      // Solver::Minimize prologue (solver.h:189-192), InitializeSolver (nelder_mead.h:94-97), Progress reset
      g[0] = 0.0;
      if constexpr (FIRST) {
        f = obj.template eval<W, 1>(x, g, n, sl);
      } else {
        f = obj.template value<W, 1>(x, n, sl);
      }
      prog.reset<W, 1>(1, x);
      make_simplex(x[0]);
    }

    // ========================= NelderMead::OptimizationStep =========================
    const double fprev = f;
    const double xprev[1] = {x[0]};
    prog.nfev += static_cast<unsigned>(nv);                     // function(simplex.col(i)) for every vertex (:111-114)
    rank_vertices();
    int best = idx[0];
    {
      // degeneracy: max over the vertices of ||v - best||_inf (:122-129)
      double far[1] = {0.0};
      if (own) {
        const double xb = S[sl + best * n];
        for (int i = 1; i < nv; ++i) {
          const double d = __builtin_fabs(S[sl + idx[i] * n] - xb);
          far[0] = (far[0] < d) ? d : far[0];
        }
      }
      const double max_dist = seg_amax<W, 1>(far);
      if (max_dist < cfg.degenerate_tol) {                 // restart around the best vertex (:130-139)
        const double xb = own ? S[sl + best * n] : 0.0;
        make_simplex(xb);
        prog.nfev += static_cast<unsigned>(nv);
        rank_vertices();
        best = idx[0];
      }
    }
    const int worst = idx[n];
    const double f_best = fv[best], f_second = fv[idx[n - 1]], f_worst = fv[worst];
    double xbar = 0.0;                                     // :142-146
    if (own) {
      for (int i = 0; i < n; ++i) xbar = xbar + S[sl + idx[i] * n];
      xbar = xbar / static_cast<double>(n);
    }
    const double xw = own ? S[sl + worst * n] : 0.0;
    const double xr = (1.0 + cfg.rho) * xbar - cfg.rho * xw;  // :149
    double dr1[1] = {xr - xbar}, dr2[1] = {xr - xw};
    bool shrink = (seg_amax<W, 1>(dr1) < cfg.degenerate_tol) || (seg_amax<W, 1>(dr2) < cfg.degenerate_tol);  // :150
    if (!shrink) {
      double xnew = xr, fnew = 0.0;
      const double f_r = value_of(xr);                     // :154
      prog.nfev += 1;
      fnew = f_r;
      if (f_r < f_best) {                                  // expansion (:156-165)
        const double xe = (1.0 + cfg.rho * cfg.xi) * xbar - (cfg.rho * cfg.xi) * xw;
        const double f_e = value_of(xe);
        prog.nfev += 1;
        if (f_e < f_r) {
          xnew = xe;
          fnew = f_e;
        }
      } else if (f_r < f_second) {                         // accept the reflected point (:166-168)
      } else if (f_r < f_worst) {                          // outside contraction (:171-180)
        const double xc = (1.0 + cfg.rho * cfg.gamma) * xbar - (cfg.rho * cfg.gamma) * xw;
        const double f_c = value_of(xc);
        prog.nfev += 1;
        if (f_c <= f_r) {
          xnew = xc;
          fnew = f_c;
        } else {
          shrink = true;
        }
      } else {                                             // inside contraction (:181-190)
        const double xc = (1.0 - cfg.gamma) * xbar + cfg.gamma * xw;
        const double f_c = value_of(xc);
        prog.nfev += 1;
        if (f_c < f_worst) {
          xnew = xc;
          fnew = f_c;
        } else {
          shrink = true;
        }
      }
      if (!shrink) {
        if (own) S[sl + worst * n] = xnew;
        if (sl == 0) fv[worst] = fnew;
      }
    }
    if (shrink) {                                          // :225-234: every vertex but the best moves towards it
      prog.nfev += static_cast<unsigned>(nv);
      const double xb = own ? S[sl + best * n] : 0.0;
      for (int i = 1; i < nv; ++i) {
        const int v = idx[i];
        if (own) S[sl + v * n] = cfg.sigma * S[sl + v * n] + (1.0 - cfg.sigma) * xb;
        evaluate_vertex(v);
      }
    }
    segment_lds_fence();
    // the step returns the vertex that was best when the step ranked them (:194); Minimize rebuilds its state
    // (solver.h:210-216): the cached value in value mode, value and gradient in first mode
    x[0] = own ? S[sl + best * n] : 0.0;
    prog.nfev += 1;
    if constexpr (FIRST) {
      f = obj.template eval<W, 1>(x, g, n, sl);
    } else {
      f = f_best;
    }

    // Progress::Update: value mode forms no gradient, so gradient_norm stays 0 and the gradient test is off (:193-196)
    prog.update<W, 1>(a.stop, stop_gradient_norm, FIRST, f, fprev, x, xprev, g, past_f, sl);
    trace_iteration<1>(a, prob, n, sl, prog.num_iterations, prog.status, f, prog.x_delta, prog.f_delta,
                       prog.gradient_norm, x, g);
    if (prog.status != MI355_STATUS_CONTINUE) {
      prog.store<1>(a, prob, n, sl, f, x, g, false);
      need_fetch = true;
    }
  }
}

}  // namespace mi355
