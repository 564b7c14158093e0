// atw_twin.hpp — TEST INFRASTRUCTURE.  The CPU twin of the ask/tell L-BFGS kernel above n = 256
// (cppnumericalsolvers_amd/csrc/lbfgs_ask_tell_wide_kernel.hpp): the same stepper — the four phases, the resumable
// More-Thuente search, the update, Progress::Update, the two-loop recursion — restated on the host over oracle::Reducer
// in its Strided order (lane t of `width` = 256 or 1024 lanes adds its terms t, t + width, ... onto 0.0, then the
// pairwise tree).  It follows the WIDE kernel's statements where they differ from the wavefront kernel's twin
// (tests/ask_tell/at_twin.hpp, whose fields, search prologue and stopping tests it reuses): a pair with |s.y| < eps is
// skipped by the recursion, not run with rho = 0; the trial point is stp * (-d) + x; the last evaluated trial — the
// caller's own buffer and gradient — is `next`.  The kernel fuses each element-wise update with the sum that follows
// it; the twin runs them one after the other: the same operations on the same operands.  Nothing here evaluates an
// objective.
#pragma once
#include "../ask_tell/at_twin.hpp"

namespace atw_twin {

using at_twin::kFinished;
using at_twin::kFirst;
using at_twin::kNoEval;
using at_twin::kTrial;

struct Problem : at_twin::Problem {
  std::vector<double> sy;  // s.y per ring slot

  void init(int n_, int m_, const double* x0) {
    at_twin::Problem::init(n_, m_, x0);
    sy.assign(m_, 0.0);
  }

  void ask_trial(double* x_eval) {
    for (int j = 0; j < n; ++j) x_eval[j] = stp * (-d[j]) + x[j];  // wa + stp * s, s = -d
    phase = kTrial;
  }

  // more_thuente.h:200-252 after the evaluation at stp gave fn and g.s = dg; 0: the search goes on, stp is the next step
  int after_evaluation(double fn, double dg) {
    const double dgtest = ftol * dginit;
    ls_nfev++;
    const double ftest1 = finit + stp * dgtest;
    int info = 0;
    if ((brackt & ((stp <= stmin) | (stp >= stmax))) | (infoc == 0)) info = 6;
    if ((stp == stpmax) & (fn <= ftest1) & (dg <= dgtest)) info = 5;
    if ((stp == stpmin) & ((fn > ftest1) | (dg >= dgtest))) info = 4;
    if (ls_nfev >= maxfev) info = 3;
    if (brackt & (stmax - stmin <= xtol * stmax)) info = 2;
    if ((fn <= ftest1) & (std::fabs(dg) <= gtol * (-dginit))) info = 1;
    if (info != 0) return info;
    if (stage1 & (fn <= ftest1) & (dg >= std::min(ftol, gtol) * dginit)) stage1 = false;
    if (stage1 & (fn <= fx) & (fn > ftest1)) {
      double fm = fn - stp * dgtest, fxm = fx - stx * dgtest, fym = fy - sty * dgtest;
      double dgm = dg - dgtest, dgxm = dgx - dgtest, dgym = dgy - dgtest;
      oracle::MoreThuente::cstep(stx, fxm, dgxm, sty, fym, dgym, stp, fm, dgm, brackt, stmin, stmax, infoc);
      fx = fxm + stx * dgtest;
      fy = fym + sty * dgtest;
      dgx = dgxm + dgtest;
      dgy = dgym + dgtest;
    } else {
      double fcur = fn, dgcur = dg;
      oracle::MoreThuente::cstep(stx, fx, dgx, sty, fy, dgy, stp, fcur, dgcur, brackt, stmin, stmax, infoc);
    }
    if (brackt) {
      if (std::fabs(sty - stx) >= 0.66 * width1) stp = stx + 0.5 * (sty - stx);
      width1 = width;
      width = std::fabs(sty - stx);
    }
    before_evaluation();
    return 0;
  }

  // one step; x_eval: the problem's row of the evaluation buffer; fin, gin: the caller's evaluation of it.
  // Returns whether the problem is still active.
  bool step(const oracle::Reducer& red, const at_stop& stop, double* x_eval, double fin, const double* gin) {
    constexpr double eps = std::numeric_limits<double>::epsilon();
    if (phase == kFinished) return false;
    std::vector<double> xn, gn;  // next, when it is not current
    double fn = 0.0;
    bool need_update = false, next_is_current = true;
    if (phase == kFirst) {
      for (int j = 0; j < n; ++j) {
        x[j] = x_eval[j];
        g[j] = gin[j];
      }
      f = fin;
      nfev = 1;
    } else {
      if (phase == kTrial) {
        fn = fin;
        nfev++;
        const double gdn = red.dot(gin, d.data(), n);  // g . d from the gradient's own pass
        if (after_evaluation(fn, -gdn) == 0) {
          ask_trial(x_eval);
          return true;
        }
        xn.assign(x_eval, x_eval + n);  // the last evaluated trial
        gn.assign(gin, gin + n);
        next_is_current = false;
      } else {  // no evaluation wanted: the refused search left next = current
        fn = f;
      }
      need_update = true;
    }

    if (need_update) {
      const double fprev = f;
      if (std::isfinite(fn)) {
        if (next_is_current) {
          xn = x;
          gn = g;
        }
        std::vector<double> sv(n), yv(n);
        for (int j = 0; j < n; ++j) {
          sv[j] = xn[j] - x[j];
          yv[j] = gn[j] - g[j];
        }
        const double sy_new = red.dot(sv.data(), yv.data(), n);
        const double ss = red.dot(sv.data(), sv.data(), n);
        const double yy = red.dot(yv.data(), yv.data(), n);
        const double sy_threshold = eps * std::sqrt(ss) * std::sqrt(yy);  // lbfgs.h:266
        if (sy_new > sy_threshold) {
          int slot;
          if (mem_count < m) {
            slot = mem_count++;
          } else {
            slot = mem_pos;
            mem_pos = (mem_pos + 1) % m;
          }
          std::copy(sv.begin(), sv.end(), S.begin() + static_cast<size_t>(slot) * n);
          std::copy(yv.begin(), yv.end(), Y.begin() + static_cast<size_t>(slot) * n);
          sy[slot] = sy_new;
        }
        if (yy > eps) {
          const double temp_scaling = sy_new / yy;
          if (std::isfinite(temp_scaling) && std::fabs(temp_scaling) <= 1e7) scaling_factor = std::max(temp_scaling, eps);
        }
        x = xn;
        g = gn;
        f = fn;
        x_delta = oracle::Reducer::amax(sv.data(), n);
      } else {
        x_delta = 0.0;  // lbfgs.h:239-241: the step returns `current`
      }
      // Progress::Update (progress.h:188-317)
      num_iterations++;
      f_delta = std::fabs(f - fprev);
      gradient_norm = oracle::Reducer::amax(g.data(), n);
      status = stop_tests(stop, fprev);
      if (status != oracle::Continue) {
        for (int j = 0; j < n; ++j) x_eval[j] = x[j];
        phase = kFinished;
        return false;
      }
    }

    // Lbfgs::OptimizationStep up to the search (lbfgs.h:89-232), pairs with |s.y| < eps skipped (:165, :189)
    const double relative_eps = eps * std::max(1.0, std::sqrt(red.dot(x.data(), x.data(), n)));
    const int k = mem_count;
    sum_k += static_cast<uint32_t>(k);
    auto slot_of = [&](int i) { return mem_count < m ? i : (mem_pos + i) % m; };
    auto active = [&](int i) { return !(std::fabs(sy[slot_of(i)]) < eps); };
    d = g;
    for (int i = k - 1; i >= 0; --i) {
      if (!active(i)) continue;
      const double* s = &S[static_cast<size_t>(slot_of(i)) * n];
      const double* y = &Y[static_cast<size_t>(slot_of(i)) * n];
      alpha[i] = (1.0 / sy[slot_of(i)]) * red.dot(s, d.data(), n);
      for (int j = 0; j < n; ++j) d[j] = d[j] - alpha[i] * y[j];
    }
    for (int j = 0; j < n; ++j) d[j] = scaling_factor * d[j];
    for (int i = 0; i < k; ++i) {
      if (!active(i)) continue;
      const double* s = &S[static_cast<size_t>(slot_of(i)) * n];
      const double* y = &Y[static_cast<size_t>(slot_of(i)) * n];
      const double beta = (1.0 / sy[slot_of(i)]) * red.dot(y, d.data(), n);
      const double c = alpha[i] - beta;
      for (int j = 0; j < n; ++j) d[j] = s[j] * c + d[j];
    }
    const double descent_direction = -red.dot(g.data(), d.data(), n);
    dginit = descent_direction;
    double alpha_init = 1.0;
    if (mem_count == 0) {
      const double dn = std::sqrt(red.dot(d.data(), d.data(), n));
      alpha_init = (dn > eps) ? 1.0 / dn : 1.0;
    }
    if (!std::isfinite(descent_direction) || descent_direction > -eps * relative_eps) {
      for (int j = 0; j < n; ++j) d[j] = -g[j];
      mem_count = 0;
      mem_pos = 0;
      const double gg = red.dot(g.data(), g.data(), n);
      const double gnorm = std::sqrt(gg);
      alpha_init = (gnorm > eps) ? 1.0 / gnorm : 1.0;
      dginit = gg;
    }
    if (dginit >= 0.0) {
      phase = kNoEval;
      return true;
    }
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
    ask_trial(x_eval);
    return true;
  }
};

// a batch: what a solve handle of the C ABI holds.  width: 256, or 1024 for n >= 32768 (the kernel's threads per problem)
struct Batch {
  int n = 0, m = 0;
  at_stop stop{};
  oracle::Reducer red;
  std::vector<Problem> problems;
  std::vector<double> x_eval;

  Batch(int n_, int m_, const at_stop& stop_, int width, int64_t B, const double* x0) : n(n_), m(m_), stop(stop_) {
    red.kind = oracle::Reduction::Strided;
    red.width = width;
    problems.resize(static_cast<size_t>(B));
    x_eval.assign(x0, x0 + B * n);
    for (int64_t b = 0; b < B; ++b) problems[static_cast<size_t>(b)].init(n, m, x0 + b * n);
  }
  int64_t tell(const double* f, const double* g) {
    int64_t active = 0;
    for (size_t b = 0; b < problems.size(); ++b)
      active += problems[b].step(red, stop, x_eval.data() + b * n, f[b], g + b * n) ? 1 : 0;
    return active;
  }
  void results(double* x, double* f, double* g, at_progress* progress) const {
    for (size_t b = 0; b < problems.size(); ++b) {
      const Problem& p = problems[b];
      for (int j = 0; j < n; ++j) {
        if (x) x[b * n + j] = p.x[j];
        if (g) g[b * n + j] = p.g[j];
      }
      if (f) f[b] = p.f;
      if (progress) progress[b] = at_progress{p.status, p.num_iterations, p.nfev, p.sum_k, p.x_delta, p.f_delta, p.gradient_norm};
    }
  }
};

}  // namespace atw_twin
