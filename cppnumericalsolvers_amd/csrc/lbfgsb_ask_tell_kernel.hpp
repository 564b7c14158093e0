// lbfgsb_ask_tell_kernel.hpp — Lbfgsb<F, m, MoreThuente>::Minimize in reverse communication: the solver state of every
// problem lives in HBM between calls, one kernel call advances every problem up to its next objective evaluation, and
// the CALLER evaluates the batch of points (torch ops, autograd, its own kernels) and hands f, g back.
//
// Device counterpart of the same reference code as lbfgsb_kernel.hpp (Lbfgsb::Minimize solver/lbfgsb.h:247-292,
// OptimizationStep :141-238, GetGeneralizedCauchyPoint :318-430, SubspaceMinimization / FindAlpha :459-515 / :435-457,
// MoreThuente::cvsrch linesearch/more_thuente.h:137-256, Progress::Update solver/progress.h:153-327), cut at its FIVE
// objective evaluations.  The statements are those of lbfgsb_solve_kernel<E, Obj, M, MI355_LS_MORE_THUENTE, NoOuterLoop,
// 16, OwnBox> and of mt_cvsrch on the same operands in the same order (its free primitives are used as they are; the
// search cut at its evaluation is MtSearch<double> of more_thuente_device.hpp), so a callback that evaluates with the
// library's own functor reproduces the persistent reference-order kernel bit for bit.
//
// Mapping: one problem per 16-lane segment (one DPP row), lane sl owns coordinates sl * E + e and row sl of the 2k x 2k
// algebra; a workgroup is one wavefront; the grid strides over the batch.  The box is read through a row stride (0: one
// box shared by the batch), so no box, a shared box and one box per problem are one code path.
//
// One call does a bounded amount of work per problem, in the order of the persistent kernel:
//   the evaluation handed back   first: the prologue;  clip-start: the clipped start of the step;  trial: the part of
//                                the cvsrch loop body after the evaluation — info == 0: the next trial point, return;
//                                cauchy: the Cauchy point;  clip-next: the clipped end of the step
//   after the search / the Cauchy evaluation: the clip test of the accepted point — outside: ask clip-next, return
//   the update                   s, y, the pair test, the chronological shift, S^T Y / S^T S, theta (history staged in
//                                LDS in the persistent kernel's layout, written back when a pair was taken),
//                                Progress::Update and the stopping tests with the projected-gradient override
//   the next step                the clip test — outside: ask clip-start, return;  sum_k, the projected gradient, MM and
//                                its LU, the Cauchy point, the subspace minimisation, FindAlpha, then the first trial
//                                of the search — or the phase "no evaluation wanted", or the ask for the Cauchy point
// No loop depends on a stopping test firing: the breakpoint loop runs at most n trips, the LU 2m.
#pragma once
#include "lbfgsb_ask_tell_config.hpp"
#include "lbfgsb_kernel.hpp"
#include "ask_tell_kernel_common.hpp"

namespace mi355 {
namespace ask_tell_box {

// One step of problem `prob` on the calling segment.  `slot`: its row of the caller's arrays (x_eval, f, g) — `prob`
// itself, or its place in the list of a compacted handle (ask_tell_compact_kernel.hpp); the state, the scalars and the
// box are indexed by `prob`.  `base`: the LDS of this segment, lbfgsb_lds_doubles_per_problem<M> doubles in the layout
// of lbfgsb_solve_kernel.  Returns the Ask the problem leaves with, kAskNothing, or kNotActive.
template <int E, int M>
__device__ __forceinline__ int step_problem(const Args& a, long long prob, long long slot, int sl, double* base) {
  using AR = ArithExact;
  constexpr int W = kLanes;
  constexpr int P = W * E;
  constexpr int K2 = 2 * M;
  static_assert(K2 <= W, "the 2M rows of the compact representation must fit the lanes of one segment");
  constexpr double kMax = 1.7976931348623157e308;

  Scalars* const sc = a.scalars + prob;
  const int phase = sc->phase;
  if (phase == kPhaseFinished) return kNotActive;

  double* const Yh = base;                  // [M][P] chronological (oldest first)
  double* const Sh = Yh + M * P;
  double* const Amat = Sh + M * P;          // S^T Y, column major, stride M
  double* const SSmat = Amat + M * M;       // S^T S
  double* const Nmat = SSmat + M * M;       // K2 x K2 scratch, column major, stride K2
  double* const LUm = Nmat + K2 * K2 + K2;  // LU of MM, row major, pitch K2
  int* const permL = reinterpret_cast<int*>(LUm + K2 * K2);
  double* const past_f = LUm + K2 * K2 + K2;

  const int n = a.n;
  const int mcap = a.m;
  double* const row = a.vectors + prob * row_doubles(mcap, M, P);
  double* const Xr = row + sl * E;
  double* const Gr = row + P + sl * E;
  double* const Dr = row + 2 * P + sl * E;
  double* const XSr = row + 3 * P + sl * E;
  double* const Yg = row + 4 * P;
  double* const Sg = Yg + static_cast<long long>(mcap) * P;
  double* const Ag = Sg + static_cast<long long>(mcap) * P;
  double* const SSg = Ag + M * M;
  const long long cbase = slot * n + sl * E;  // of the caller's [B][n] arrays

  double lo[E], hi[E];
  {
    const long long brow = prob * a.box_stride;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = sl * E + e;
      lo[e] = (j < n) ? a.lower[brow + j] : 0.0;
      hi[e] = (j < n) ? a.upper[brow + j] : 0.0;
    }
  }
  auto clip = [&](const double (&v)[E], double (&out)[E]) {  // cwiseMin(upper).cwiseMax(lower)
#pragma unroll
    for (int e = 0; e < E; ++e) out[e] = dmax(dmin(v[e], hi[e]), lo[e]);
  };
  auto differs = [&](const double (&u)[E], const double (&v)[E]) {
    int dflag = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) dflag |= (sl * E + e < n && u[e] != v[e]) ? 1 : 0;
    return seg_max<W>(static_cast<double>(dflag)) != 0.0;
  };
  auto load_vec = [&](const double* p, double (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = p[e];
  };
  auto store_vec = [&](double* p, const double (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) p[e] = v[e];
  };
  auto load_caller_g = [&](double (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = (sl * E + e < n) ? a.g[cbase + e] : 0.0;
  };
  auto store_x_eval = [&](const double (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (sl * E + e < n) a.x_eval[cbase + e] = v[e];
  };

  // what the persistent kernel keeps in registers across iterations
  double x[E], g[E];
  double f = 0.0;
  unsigned nfev = 0, sum_k = 0;
  int k = 0;
  double theta = 1.0;
  double mm_row[K2];
  int mm_perm = 0;
  double last_pg = 0.0;
  unsigned num_iterations = 0;
  int x_delta_violations = 0, f_delta_violations = 0;
  double x_delta = 0.0, f_delta = 0.0, gradient_norm = 0.0;
  int status = MI355_STATUS_NOT_STARTED;
  bool past_init = false;
  int past_pos = 0;
  double f_state = 0.0;
#pragma unroll
  for (int j = 0; j < K2; ++j) mm_row[j] = 0.0;

  MtSearch<double> mt;  // the running search, segment-uniform

  // everything but the search's scalars; f_store: the value at X (the returned f once finished)
  auto store_scalars = [&](int next_phase, double f_store) {
    if (sl == 0) {
      sc->f = f_store; sc->f_state = f_state; sc->theta = theta; sc->last_pg = last_pg;
      sc->x_delta = x_delta; sc->f_delta = f_delta; sc->gradient_norm = gradient_norm;
      sc->k = k; sc->status = status;
      sc->x_delta_violations = x_delta_violations; sc->f_delta_violations = f_delta_violations;
      sc->past_init = past_init; sc->past_pos = past_pos;
      sc->nfev = nfev; sc->sum_k = sum_k; sc->num_iterations = num_iterations;
      sc->phase = next_phase;
    }
  };
  // the trial point wa + stp s = wa - stp d into the evaluation buffer, and the search's scalars
  auto ask_trial = [&](const double (&wa)[E], const double (&d)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (sl * E + e < n) a.x_eval[cbase + e] = AR::nmadd(mt.stp, d[e], wa[e]);
    if (sl == 0) {
      mt.store(sc);
      sc->nfev = nfev;
      sc->phase = kPhaseTrial;
    }
  };

  // where the call goes on after the evaluation it was handed
  enum Stage { kStartStep, kDirection, kAfterSearch, kUpdate };
  int stage;
  double xcur[E], gcur[E];  // the iterate the step started from, after the clip (s and y are taken against it)
  double fcur = 0.0;

  if (phase == kPhaseFirst) {
    // ---- Minimize's prologue (:253) + InitializeSolver (:120-139): the caller's f, g are the evaluation at x0 --------
    load_vec(Xr, x);  // (x0, put there by the state initialisation)
    load_caller_g(g);
    f = a.f[slot];
    nfev = 1;  // reset_solver of lbfgsb_kernel.hpp: everything else is the initial value above
    stage = kStartStep;
  } else {
    f_state = sc->f_state; theta = sc->theta; last_pg = sc->last_pg;
    x_delta = sc->x_delta; f_delta = sc->f_delta; gradient_norm = sc->gradient_norm;
    k = sc->k; status = sc->status;
    x_delta_violations = sc->x_delta_violations; f_delta_violations = sc->f_delta_violations;
    past_init = sc->past_init != 0; past_pos = sc->past_pos;
    nfev = sc->nfev; sum_k = sc->sum_k; num_iterations = sc->num_iterations;
    if (phase == kPhaseClipStart) {
      // ---- the evaluation at clip(x) (:151-153) ----------------------------------------------------------------------
      load_vec(Xr, x);
      load_caller_g(g);
      f = a.f[slot];
      nfev++;
      stage = kDirection;
    } else {
      load_vec(Xr, xcur);
      load_vec(Gr, gcur);
      fcur = sc->f;
      if (phase == kPhaseTrial) {
        // ---- the cvsrch loop body after the evaluation (more_thuente.h:200-252) --------------------------------------
        double d[E], gn[E];
        load_vec(Dr, d);
        load_caller_g(gn);
        const double fn = a.f[slot];
        mt.load(sc);
        if (mt.after_evaluation(fn, [&]() { nfev++; return -seg_dot<W, E, AR>(gn, d); }) == 0) {  // (g.s)
          ask_trial(xcur, d);
          return kAskTrial;
        }
        // the search ended: the accepted point, re-formed from the accepted step (as mt_cvsrch ends)
#pragma unroll
        for (int e = 0; e < E; ++e) {
          x[e] = AR::nmadd(mt.stp, d[e], xcur[e]);
          g[e] = gn[e];
        }
        f = fn;
        stage = kAfterSearch;
      } else if (phase == kPhaseNoEval) {
        // ---- no evaluation wanted: the refused search left x, f, g untouched ------------------------------------------
#pragma unroll
        for (int e = 0; e < E; ++e) {
          x[e] = xcur[e];
          g[e] = gcur[e];
        }
        f = fcur;
        stage = kAfterSearch;
      } else {
        // ---- the evaluation at the Cauchy point (:191-193) or at clip(next.x) (:199-203): the point is vector D -------
        load_vec(Dr, x);
        load_caller_g(g);
        f = a.f[slot];
        nfev++;
        stage = (phase == kPhaseCauchy) ? kAfterSearch : kUpdate;
      }
    }
  }

  if (stage == kAfterSearch) {
    double xcl[E];
    clip(x, xcl);                                                     // :199-203
    if (differs(xcl, x)) {
      store_vec(Dr, xcl);
      store_x_eval(xcl);
      store_scalars(kPhaseClipNext, fcur);
      return kAskClipNext;
    }
    stage = kUpdate;
  }

  // the histories and S^T Y / S^T S of this problem staged in LDS (the persistent kernel's layout)
  auto load_history = [&]() {
    for (int col = 0; col < k; ++col) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        Yh[col * P + sl * E + e] = Yg[col * P + sl * E + e];
        Sh[col * P + sl * E + e] = Sg[col * P + sl * E + e];
      }
    }
#pragma unroll
    for (int r = 0; r < (M * M + W - 1) / W; ++r) {
      const int idx = sl + r * W;
      if (idx < M * M && idx % M < k && idx / M < k) {
        Amat[idx] = Ag[idx];
        SSmat[idx] = SSg[idx];
      }
    }
    segment_lds_fence();
  };
  bool staged = false;

  if (stage == kUpdate) {
    // ---- history / compact representation update (:206-235) -----------------------------------------------------------
    load_history();
    staged = true;
    {
      double ny[E], ns[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        ny[e] = g[e] - gcur[e];
        ns[e] = x[e] - xcur[e];
      }
      const double sTy = seg_dot<W, E>(ns, ny);
      const double yTy = seg_dot<W, E>(ny, ny);
      if (sTy > 1e-7 * yTy) {                                         // :211
        if (k < mcap) {
          k++;
        } else {                                                      // shift left (:216-217)
          for (int col = 0; col + 1 < mcap; ++col) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
              Yh[col * P + sl * E + e] = Yh[(col + 1) * P + sl * E + e];
              Sh[col * P + sl * E + e] = Sh[(col + 1) * P + sl * E + e];
            }
          }
          // S^T Y and S^T S lose their first row and column
          double ta[(M * M + W - 1) / W], ts[(M * M + W - 1) / W];
#pragma unroll
          for (int r = 0; r < (M * M + W - 1) / W; ++r) {
            const int idx = sl + r * W;
            const int ia = idx % M, ib = idx / M;
            const bool ok = idx < M * M && ia + 1 < mcap && ib + 1 < mcap;
            ta[r] = ok ? Amat[(ib + 1) * M + ia + 1] : 0.0;
            ts[r] = ok ? SSmat[(ib + 1) * M + ia + 1] : 0.0;
          }
          segment_lds_fence();
#pragma unroll
          for (int r = 0; r < (M * M + W - 1) / W; ++r) {
            const int idx = sl + r * W;
            const int ia = idx % M, ib = idx / M;
            if (idx < M * M && ia + 1 < mcap && ib + 1 < mcap) {
              Amat[ib * M + ia] = ta[r];
              SSmat[ib * M + ia] = ts[r];
            }
          }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
          Yh[(k - 1) * P + sl * E + e] = ny[e];
          Sh[(k - 1) * P + sl * E + e] = ns[e];
        }
        segment_lds_fence();
        theta = yTy / sTy;                                            // :222-223 (y.s == s.y bit for bit)
        // new column / row of S^T Y, new row+column of S^T S (older entries are unchanged)
        {
          // value 3*col + {0,1,2}: S_col.y_new, s_new.Y_col, S_col.s_new — one transposed butterfly
          double part[3 * M];
#pragma unroll
          for (int col = 0; col < M; ++col) {
            double t0[E], t1[E], t2[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const double scol = (col < k) ? Sh[col * P + sl * E + e] : 0.0;
              const double ycol = (col < k) ? Yh[col * P + sl * E + e] : 0.0;
              t0[e] = scol * ny[e];
              t1[e] = ns[e] * ycol;
              t2[e] = scol * ns[e];
            }
            part[3 * col + 0] = lane_tree_sum<E>(t0);
            part[3 * col + 1] = lane_tree_sum<E>(t1);
            part[3 * col + 2] = lane_tree_sum<E>(t2);
          }
          auto store = [&](int idx, double val) {
            const int col = idx / 3, which = idx - 3 * col;
            if (idx < 3 * M && col < k) {
              if (which == 0) Amat[(k - 1) * M + col] = val;          // A(col, k-1) = S_col . y_new
              if (which == 1) Amat[col * M + (k - 1)] = val;          // A(k-1, col) = s_new . Y_col
              if (which == 2) {                                       // SS(col, k-1) = SS(k-1, col)
                SSmat[(k - 1) * M + col] = val;
                SSmat[col * M + (k - 1)] = val;
              }
            }
          };
          if constexpr (3 * M <= W) {
            store(sl, row_transpose_sum<3 * M, W>(part, sl));
          } else {  // more sums than lanes (M = 8: 24): two transposed butterflies, the same pairwise trees
            static_assert(3 * M <= 2 * W, "history size");
            double p0[W], p1[3 * M - W];
#pragma unroll
            for (int i = 0; i < W; ++i) p0[i] = part[i];
#pragma unroll
            for (int i = 0; i < 3 * M - W; ++i) p1[i] = part[W + i];
            const double v0 = row_transpose_sum<W, W>(p0, sl);
            const double v1 = row_transpose_sum<3 * M - W, W>(p1, sl);
            store(sl, v0);
            store(W + sl, v1);
          }
        }
        segment_lds_fence();
        // the state row takes the new histories (a lane writes its own coordinates; the matrices lane by index)
        for (int col = 0; col < k; ++col) {
#pragma unroll
          for (int e = 0; e < E; ++e) {
            Yg[col * P + sl * E + e] = Yh[col * P + sl * E + e];
            Sg[col * P + sl * E + e] = Sh[col * P + sl * E + e];
          }
        }
#pragma unroll
        for (int r = 0; r < (M * M + W - 1) / W; ++r) {
          const int idx = sl + r * W;
          if (idx < M * M && idx % M < k && idx / M < k) {
            Ag[idx] = Amat[idx];
            SSg[idx] = SSmat[idx];
          }
        }
        // (MM and its LU, :227-234, are formed where the next step needs them: below)
      }
    }

    // ================== Progress::Update (progress.h:153-327), gradient test off ==========
    double xs[E];
    load_vec(XSr, xs);
    const mi355_lbfgs_stop& st = a.stop;
    if (st.past > 0) {
      if (past_init && sl < st.past) past_f[sl] = sc->past_f[sl];
      segment_lds_fence();
    }
    num_iterations++;
    f_delta = __builtin_fabs(f - f_state);
    {
      double dx[E];
#pragma unroll
      for (int e = 0; e < E; ++e) dx[e] = x[e] - xs[e];
      x_delta = seg_amax<W, E>(dx);
    }
    gradient_norm = seg_amax<W, E>(g);
    status = MI355_STATUS_CONTINUE;
    bool decided = false;
    if ((st.num_iterations > 0) && (num_iterations > st.num_iterations)) {
      status = MI355_STATUS_ITERATION_LIMIT;
      decided = true;
    }
    if (!decided) {
      if ((st.x_delta > 0) && (x_delta < st.x_delta)) {
        x_delta_violations++;
        if (x_delta_violations >= st.x_delta_violations) {
          status = MI355_STATUS_X_DELTA_VIOLATION;
          decided = true;
        }
      } else {
        x_delta_violations = 0;
      }
    }
    if (!decided) {
      const double fscale =
          st.f_delta_relative ? dmax(dmax(__builtin_fabs(f), __builtin_fabs(f_state)), 1.0) : 1.0;
      if ((st.f_delta > 0) && (f_delta < st.f_delta * fscale)) {
        f_delta_violations++;
        if (f_delta_violations >= st.f_delta_violations) {
          status = MI355_STATUS_F_DELTA_VIOLATION;
          decided = true;
        }
      } else {
        f_delta_violations = 0;
      }
    }
    if (!decided && st.past > 0) {
      const int pw = st.past;
      if (!past_init) {
        if (sl < pw) past_f[sl] = f;
        past_init = true;
        past_pos = 0;
        segment_lds_fence();
      }
      if (static_cast<int>(num_iterations) > pw) {
        const double pf = past_f[past_pos];
        const double rate = __builtin_fabs(pf - f) / dmax(1.0, __builtin_fabs(f));
        if (rate < st.past_delta) {
          status = MI355_STATUS_F_DELTA_VIOLATION;
          decided = true;
        }
      }
      if (!decided) {
        if (sl == 0) past_f[past_pos] = f;
        segment_lds_fence();
        past_pos = (past_pos + 1 == pw) ? 0 : past_pos + 1;
      }
    }
    if (st.past > 0 && past_init) {
      segment_lds_fence();
      if (sl < st.past) sc->past_f[sl] = past_f[sl];
    }
    // projected-gradient stop (:280-283): overrides whatever Update decided (quirk Q10)
    if ((st.gradient_norm > 0) && (last_pg < st.gradient_norm)) status = MI355_STATUS_GRADIENT_NORM_VIOLATION;

    if (status != MI355_STATUS_CONTINUE) {
      // finished: frozen from here on; the evaluation buffer holds the returned x
      store_vec(Xr, x);
      store_vec(Gr, g);
      store_x_eval(x);
      store_scalars(kPhaseFinished, f);
      return kNotActive;
    }
    stage = kStartStep;
  }

  // ============================ OptimizationStep (:141-238) ===========================
  if (stage == kStartStep) {
    f_state = f;
    store_vec(XSr, x);  // state x at entry (Progress::Update compares against it)
    double xc0[E];
    clip(x, xc0);                                                     // :148
    if (differs(xc0, x)) {                                            // :151-153
      store_vec(Xr, xc0);
      store_x_eval(xc0);
      store_scalars(kPhaseClipStart, f);
      return kAskClipStart;
    }
  }
  if (!staged) load_history();
  const int k2 = 2 * k;
  if (k2 > 0) {
    // MM = [[-diag(A), L^T], [L, theta*S^T S]] (:227-232): lane i assembles row i, then LU (:234)
#pragma unroll
    for (int j = 0; j < K2; ++j) {
      double val = 0.0;
      if (sl < k2 && j < k2) {
        const int i = sl;
        if (i < k && j < k) {
          val = (i == j) ? -1 * Amat[i * M + i] : 0.0;
        } else if (i < k && j >= k) {
          const int jj = j - k;  // L^T(i, jj) = L(jj, i)
          val = (jj > i) ? Amat[i * M + jj] : 0.0;
        } else if (i >= k && j < k) {
          const int ii = i - k;  // L(ii, j)
          val = (ii > j) ? Amat[j * M + ii] : 0.0;
        } else {
          val = SSmat[(j - k) * M + (i - k)] * theta;
        }
      }
      mm_row[j] = val;
    }
    lu_factor<K2, W>(mm_row, mm_perm, k2, sl);
    if (sl < k2) {  // LDS copy for the side-by-side column solves
#pragma unroll
      for (int j = 0; j < K2; ++j) LUm[sl * K2 + j] = mm_row[j];
      permL[sl] = mm_perm;
    }
    segment_lds_fence();
  }

  auto Wval = [&](int col, int coord) {  // W = [Y, theta*S]  (:224-226)
    const bool is_y = col < k;
    const int column = is_y ? col : (M + col - k);
    const double scale = is_y ? 1.0 : theta;
    return scale * Yh[column * P + coord];
  };
  auto solveM = [&](double v, int kk2) {  // :311-316
    return (kk2 == 0) ? v : lu_solve<K2, W>(mm_row, mm_perm, kk2, sl, v);
  };

  sum_k += k;
  {  // projected gradient sup-norm (:105-118, :165-166)
    double t[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      double gj = g[e];
      if (x[e] <= lo[e] && gj > 0) gj = 0.0;
      if (x[e] >= hi[e] && gj < 0) gj = 0.0;
      t[e] = (sl * E + e < n) ? __builtin_fabs(gj) : 0.0;
    }
    last_pg = seg_max<W>(lane_max<E>(t));
  }

  // ---- generalized Cauchy point (:318-430) -------------------------------------------
  double xc[E], d[E], tb[E];
  bool pending[E];
  double c_vec = 0.0, p_vec = 0.0;  // distributed 2k-vectors
  {
    int npos = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = sl * E + e;
      d[e] = -g[e];
      double tmp = kMax;
      if (g[e] != 0) {
        tmp = (g[e] < 0) ? (x[e] - hi[e]) / g[e] : (x[e] - lo[e]) / g[e];
        if (tmp == 0) d[e] = 0;
      }
      tb[e] = tmp;
      xc[e] = x[e];
      pending[e] = (j < n) && (tmp > 0);
      npos += pending[e] ? 1 : 0;
      if (j >= n) d[e] = 0.0;
    }
    const bool any_positive = seg_max<W>(static_cast<double>(npos)) > 0.0;
    {                                                               // p = W^T d (:353)
      double part[K2];  // all 2k dot products share one transposed butterfly
#pragma unroll
      for (int col = 0; col < K2; ++col) {
        double t[E];
#pragma unroll
        for (int e = 0; e < E; ++e) t[e] = (col < k2) ? Wval(col, sl * E + e) * d[e] : 0.0;
        part[col] = lane_tree_sum<E>(t);
      }
      const double val = row_transpose_sum<K2, W>(part, sl);
      p_vec = (sl < k2) ? val : 0.0;
    }
    double f_prime = -seg_dot<W, E>(d, d);                           // :357
    const double Mp0 = solveM(p_vec, k2);
    const double pMp = row_seq_sum<K2, W>(p_vec * Mp0, k2);
    double f_doubleprime = (-theta) * f_prime - pMp;                // :361-362
    f_doubleprime = dmax(1e-12, f_doubleprime);
    const double f_dp_orig = f_doubleprime;
    double dt_min = -f_prime / f_doubleprime;
    double t_old = 0.0;

    // breakpoint selection by (t, index) key among a candidate set
    auto select_min = [&](const bool (&cand)[E], int& b_out, double& t_out) {
      double bt = kMax;
      int bj = 0x7fffffff;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = sl * E + e;
        if (cand[e] && (tb[e] < bt || (tb[e] == bt && j < bj))) {
          bt = tb[e];
          bj = j;
        }
      }
      // lanes without a candidate must not win: key (kMax, INT_MAX)
      const double tmin = row_min_select<W>(bj == 0x7fffffff ? kMax : bt);
      const int jmin = row_min_i<W>((bj != 0x7fffffff && bt == tmin) ? bj : 0x7fffffff);
      b_out = jmin;
      t_out = tmin;
    };
    int b = 0;
    double t = 0.0;
    int remaining;  // entries at sorted positions >= i
    if (any_positive) {
      select_min(pending, b, t);
      remaining = static_cast<int>(seg_sum<W>(static_cast<double>(npos)));
    } else {
      // all t <= 0: the reference lands on the LAST sorted entry (:370-375): max (t, index)
      double bt = -kMax;
      int bj = -1;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = sl * E + e;
        if (j < n && (tb[e] > bt || (tb[e] == bt && j > bj))) {
          bt = tb[e];
          bj = j;
        }
      }
      const double tmax = seg_max<W>(bj < 0 ? -kMax : bt);
      const int jmax = -row_min_i<W>((bj >= 0 && bt == tmax) ? -bj : 0x7fffffff);
      b = jmax;
      t = tmax;
      remaining = 1;
#pragma unroll
      for (int e = 0; e < E; ++e) pending[e] = (sl * E + e == b);
    }
    double dt = t;
    // (at most n trips: every trip takes one breakpoint out of `remaining` <= n)
    while ((dt_min >= dt) && (remaining > 0)) {                     // :382-412
      const int owner = b / E, be = b % E;
      double gsel = 0.0, dsel = 0.0, xsel = 0.0, losel = 0.0, hisel = 0.0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (e == be) {
          gsel = g[e];
          dsel = d[e];
          xsel = x[e];
          losel = lo[e];
          hisel = hi[e];
        }
      }
      const double gb = row_bcast_dyn<W>(gsel, owner);
      const double db = row_bcast_dyn<W>(dsel, owner);
      const double xb = row_bcast_dyn<W>(xsel, owner);
      const double lob = row_bcast_dyn<W>(losel, owner);
      const double hib = row_bcast_dyn<W>(hisel, owner);
      double xcb = xb;
      if (db > 0)
        xcb = hib;
      else if (db < 0)
        xcb = lob;
      const double zb = xcb - xb;
      c_vec = c_vec + dt * p_vec;
      const double wbt = (sl < k2) ? Wval(sl, b) : 0.0;            // W.row(b): lane a reads W(b, a)
      // M^-1 c, M^-1 p, M^-1 W.row(b): three right-hand sides, solved side by side (lanes 0..2)
      double Mc = c_vec, Mp = p_vec, Mwbt = wbt;
      if (k2 > 0) {
        if (sl < k2) {
          Nmat[0 * K2 + sl] = c_vec;
          Nmat[1 * K2 + sl] = p_vec;
          Nmat[2 * K2 + sl] = wbt;
        }
        segment_lds_fence();
        lu_solve_columns<K2>(LUm, permL, Nmat, k2, 3, sl, 0);
        segment_lds_fence();
        Mc = (sl < k2) ? Nmat[0 * K2 + sl] : 0.0;
        Mp = (sl < k2) ? Nmat[1 * K2 + sl] : 0.0;
        Mwbt = (sl < k2) ? Nmat[2 * K2 + sl] : 0.0;
        segment_lds_fence();
      }
      const double s1 = row_seq_sum<K2, W>((gb * wbt) * Mc, k2);
      const double s2 = row_seq_sum<K2, W>(wbt * Mp, k2);
      const double s3 = row_seq_sum<K2, W>(((gb * gb) * wbt) * Mwbt, k2);
      f_prime += ((dt * f_doubleprime + gb * gb) + (theta * gb) * zb) - s1;        // :396-397
      f_doubleprime += ((((-1.0) * theta) * gb) * gb - 2.0 * (gb * s2)) - s3;      // :398-400
      f_doubleprime = dmax(1e-12 * f_dp_orig, f_doubleprime);
      p_vec = p_vec + gb * wbt;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (sl * E + e == b) {
          xc[e] = xcb;
          d[e] = 0.0;
          pending[e] = false;
        }
      }
      dt_min = -f_prime / f_doubleprime;
      t_old = t;
      remaining--;
      if (remaining > 0) {
        select_min(pending, b, t);
        dt = t - t_old;
      }
    }
    dt_min = dmax(dt_min, 0.0);
    t_old += dt_min;
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (pending[e]) xc[e] = x[e] + t_old * d[e];                  // :424-427
    c_vec = c_vec + dt_min * p_vec;                                 // :429
  }

  // ---- subspace minimisation (:459-515) -----------------------------------------------
  double smin[E];
  bool do_line_search;
  {
    bool is_free[E];
    int nfree = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      is_free[e] = (sl * E + e < n) && (xc[e] != hi[e]) && (xc[e] != lo[e]);
      nfree += is_free[e] ? 1 : 0;
      smin[e] = xc[e];
    }
    do_line_search = seg_max<W>(static_cast<double>(nfree)) > 0.0;
    if (do_line_search) {
      const double theta_inverse = 1.0 / theta;
      const double Mc = solveM(c_vec, k2);
      double rr[E];
      {
        double wmc[E];
#pragma unroll
        for (int e = 0; e < E; ++e) wmc[e] = 0.0;
        static_for<0, K2>([&](auto ic) {
          constexpr int col = decltype(ic)::value;
          const double mca = row_bcast<W, col>(Mc);
          if (col < k2) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const double term = Wval(col, sl * E + e) * mca;
              wmc[e] = (col == 0) ? term : wmc[e] + term;
            }
          }
        });
#pragma unroll
        for (int e = 0; e < E; ++e) rr[e] = (g[e] + theta * (xc[e] - x[e])) - wmc[e];   // :480
      }
      double wzr;
      {                                                             // WZ * r (:485)
        double part[K2];
#pragma unroll
        for (int col = 0; col < K2; ++col) {
          double t[E];
#pragma unroll
          for (int e = 0; e < E; ++e) t[e] = (col < k2 && is_free[e]) ? Wval(col, sl * E + e) * rr[e] : 0.0;
          part[col] = lane_tree_sum<E>(t);
        }
        const double val = row_transpose_sum<K2, W>(part, sl);
        wzr = (sl < k2) ? val : 0.0;
      }
      // v = M^-1 (WZ r) (:486).  Where a lane of the segment is left over (2k < 16) the solve rides along with the
      // column solves of N = I - M^-1 N below as one more column — same factors, same operation order as lu_solve.
      constexpr bool kRideAlong = (K2 < W);
      double v = (kRideAlong && k2 > 0) ? 0.0 : solveM(wzr, k2);
      // N = theta^-1 WZ WZ^T (:487), then N = I - M^-1 N (:489-495), built in LDS
      {
        double Um[K2][E];
#pragma unroll
        for (int ar = 0; ar < K2; ++ar) {
#pragma unroll
          for (int e = 0; e < E; ++e)
            Um[ar][e] = (ar < k2 && is_free[e]) ? theta_inverse * Wval(ar, sl * E + e) : 0.0;
        }
        constexpr int kTotal = K2 * K2;
        constexpr int kBatch = W;
        constexpr int kBatches = (kTotal + kBatch - 1) / kBatch;
        static_for<0, kBatches>([&](auto ib) {
          constexpr int first = decltype(ib)::value * kBatch;
          constexpr int cnt = (kTotal - first < kBatch) ? (kTotal - first) : kBatch;
          constexpr int bc_lo = first / K2, bc_hi = (first + cnt - 1) / K2;
          if (bc_lo < k2) {
            double wbm[bc_hi - bc_lo + 1][E];
#pragma unroll
            for (int c = 0; c <= bc_hi - bc_lo; ++c) {
              const int col = (bc_lo + c < k2) ? bc_lo + c : 0;
#pragma unroll
              for (int e = 0; e < E; ++e)
                wbm[c][e] = (is_free[e] && bc_lo + c < k2) ? Wval(col, sl * E + e) : 0.0;
            }
            double part[cnt];
#pragma unroll
            for (int i = 0; i < cnt; ++i) {
              const int bc = (first + i) / K2, ar = (first + i) % K2;
              double t[E];
#pragma unroll
              for (int e = 0; e < E; ++e) t[e] = Um[ar][e] * wbm[bc - bc_lo][e];
              part[i] = lane_tree_sum<E>(t);
            }
            const double val = row_transpose_sum<cnt, W>(part, sl);
            const int slo = opaque_lane(sl);
            const int idx = first + slo;
            if (slo < cnt && (idx % K2) < k2 && (idx / K2) < k2) Nmat[idx] = val;
          }
        });
      }
      if (kRideAlong && k2 > 0 && sl < k2) Nmat[k2 * K2 + sl] = wzr;
      segment_lds_fence();
      if (k2 > 0)  // N = I - M^-1 N, column per lane (+ the ride-along right-hand side)
        lu_solve_columns<K2>(LUm, permL, Nmat, k2, kRideAlong ? k2 + 1 : k2, sl, k2);
      segment_lds_fence();
      if (k2 > 0) {                                                 // :498-500
        double nrow[K2];
        int nperm = 0;
#pragma unroll
        for (int j = 0; j < K2; ++j) nrow[j] = (sl < k2 && j < k2) ? Nmat[j * K2 + sl] : 0.0;
        if constexpr (kRideAlong) v = (sl < k2) ? Nmat[k2 * K2 + sl] : 0.0;
        lu_factor<K2, W>(nrow, nperm, k2, sl);
        v = lu_solve<K2, W>(nrow, nperm, k2, sl, v);
      }
      const double ti2 = theta_inverse * theta_inverse;
      double du[E];
      {
        double wv[E];
#pragma unroll
        for (int e = 0; e < E; ++e) wv[e] = 0.0;
        static_for<0, K2>([&](auto ic) {
          constexpr int col = decltype(ic)::value;
          const double va = row_bcast<W, col>(v);
          if (col < k2) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const double term = (ti2 * Wval(col, sl * E + e)) * va;
              wv[e] = (col == 0) ? term : wv[e] + term;
            }
          }
        });
#pragma unroll
        for (int e = 0; e < E; ++e) du[e] = (-theta_inverse) * rr[e] - wv[e];   // :503-504
      }
      double amin = 1.0;                                            // FindAlpha (:435-457)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (is_free[e] && !(__builtin_fabs(du[e]) < 1e-7)) {
          const double cand = (du[e] > 0) ? (hi[e] - xc[e]) / du[e] : (lo[e] - xc[e]) / du[e];
          amin = dmin(amin, cand);
        }
      }
      const double alphastar = row_min_select<W>(amin);
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (is_free[e]) smin[e] = smin[e] + alphastar * du[e];      // :508-514
    }
  }
  segment_lds_fence();  // (the LDS of this segment is rewritten by its next problem)

  // ---- line search / evaluation (:181-203): the iterate the step starts from becomes the state -------------------------
  store_vec(Xr, x);
  store_vec(Gr, g);
  if (!do_line_search) {
    store_vec(Dr, smin);
    store_x_eval(smin);
    store_scalars(kPhaseCauchy, f);
    return kAskCauchy;
  }
  double dneg[E];  // negated direction (mt_cvsrch runs along -dneg)
#pragma unroll
  for (int e = 0; e < E; ++e) dneg[e] = -(smin[e] - x[e]);
  const double dginit = -seg_dot<W, E>(g, dneg);
  store_vec(Dr, dneg);
  if (dginit >= 0.0) {  // more_thuente.h:152-156: no evaluation; the next call finishes this iteration
    store_scalars(kPhaseNoEval, f);
    return kAskNothing;
  }
  // ---- the search starts (more_thuente.h:158-177) and asks for its first trial -----------------------------------------
  store_scalars(kPhaseTrial, f);
  mt.start(f, dginit, 1.0);
  ask_trial(x, dneg);
  return kAskTrial;
}

// dynamic LDS of a step kernel: one segment's layout of lbfgsb_solve_kernel per segment of the wavefront
template <int E, int M>
__host__ __device__ inline int segment_lds_doubles() {
  return lbfgsb_lds_doubles_per_problem<M>(kLanes * E, 0);
}
template <int E, int M>
inline int step_lds_bytes() {
  return (kWave / kLanes) * segment_lds_doubles<E, M>() * static_cast<int>(sizeof(double));
}

// One step of every row a.B counts, the tally of the problems still active after it and of what they ask for.  Dense
// (kListed false): row r is problem r and a.B the batch.  Listed: row s of x_eval / f / g belongs to problem ids[s],
// ids ascending, a.B is the LENGTH OF THE LIST (nothing of a step is indexed by the batch size) and the grid is sized
// from it.  The grid loop is spelled here, as in the run_steps of the two Lbfgs paths, and Args comes by value: handed to
// a shared function as a callback that tallies through captured references, the loop cost the kernels at two and four
// coordinates per lane 8 to 26 registers; as a shared loop object, two in the listed kernels; Args by reference, two in
// step_kernel<4, 5> (profiles/ask_tell_box_kernel_resources.txt).
template <int E, int M, bool kListed>
__device__ __forceinline__ void run_steps(const Args a, const long long* ids) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int W = kLanes;
  constexpr int kSegs = kWave / W;
  const int lane = threadIdx.x;
  const int seg = lane / W;
  const int sl = lane % W;
  double* const base = lds + seg * segment_lds_doubles<E, M>();
  unsigned long long active_count = 0;  // wavefront-uniform
  unsigned long long ask_count[kAskKinds - 1] = {0, 0, 0, 0};
  const long long stride = static_cast<long long>(gridDim.x) * kSegs;
  for (long long first = static_cast<long long>(blockIdx.x) * kSegs; first < a.B; first += stride) {
    const long long slot = first + seg;
    int ask = kNotActive;
    if (slot < a.B) ask = step_problem<E, M>(a, kListed ? ids[slot] : slot, slot, sl, base);
    const bool lead = sl == 0;
    active_count += __builtin_popcountll(__builtin_amdgcn_ballot_w64(lead && ask != kNotActive));
#pragma unroll
    for (int kind = 0; kind < kAskKinds - 1; ++kind)
      ask_count[kind] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(lead && ask == kind));
  }
  if (lane == 0) {
    if (active_count != 0) atomicAdd(a.active, active_count);
#pragma unroll
    for (int kind = 0; kind < kAskKinds - 1; ++kind)
      if (ask_count[kind] != 0) atomicAdd(a.asks + kind, ask_count[kind]);
  }
}

// The two entry points of run_steps: two kernels, so that the dense one takes no list argument and tests none.
template <int E, int M>
__global__ __launch_bounds__(64) void step_kernel(const Args a) {
  run_steps<E, M, false>(a, nullptr);
}

template <int E, int M>
__global__ __launch_bounds__(64) void listed_step_kernel(const Args a, const long long* ids) {
  run_steps<E, M, true>(a, ids);
}

// (the state initialisation is dispatch_lbfgsb_ask_tell.hip's, the result gather ask_tell_kernel_common.hpp's)

}  // namespace ask_tell_box
}  // namespace mi355
