// more_thuente_device.hpp — Moré–Thuente line search on a wavefront segment, for ScalarType double and float.
//
// Device counterpart of the reference's linesearch/more_thuente.h:
//   Search (State overload)  :120-135
//   cvsrch                   :137-256   MtSearch<T>: the scalar state of one search and the halves of the loop body
//   cstep                    :261-407   mt_cstep<T>
// All step-length bookkeeping (stx, fx, dgx, sty, ... ) is scalar and
// segment-uniform: every lane of the segment carries the same value and takes
// the same branch, so the control flow below is the reference's own, executed
// redundantly per lane; only the trial point x = wa + stp*s, the objective and
// the directional derivative dg = g.s are lane-parallel.
//
// cstep has ONE body, mt_cstep<T>, and the constants one home, MtSearch<T>.  Every constant is static_cast<T>(double
// literal), the double literal rounded once, as the reference forms ScalarType(1e-4) — never an f-suffixed literal; the
// units are built with -ffp-contract=off and every path relies on the operand order of the expressions below, so the
// persistent kernels, the ask/tell kernels and a caller that evaluates with the library's own functor agree bit for bit.
//
// MtSearch<T> is the search of mt_cvsrch_peeled below (the lean kernels), lbfgs_wide_kernel.hpp, ridge_mfma_kernel.hpp
// and the three ask/tell step kernels.  What stays with those, because it differs per path: forming the trial point
// from stp, the evaluation and where dg = g.s comes from, the barrier, re-forming the accepted point.
// mt_cvsrch and f32::mt_cvsrch spell cvsrch's loop out over mt_cstep<T> and the shared constants: as drivers of
// MtSearch the general and float kernels took more registers, some a wavefront per SIMD fewer, some scratch
// (profiles/more_thuente_one_search_resources.txt).  A change to the loop body is made in MtSearch and in those two.
#pragma once
#include "wave_primitives.hpp"
#include "wave_primitives_f32.hpp"

namespace mi355 {

// std::min / std::max / std::clamp as the reference's expressions evaluate them (which operand a NaN or a tie returns)
template <class T>
__device__ __forceinline__ T std_min(T a, T b) { return (b < a) ? b : a; }
template <class T>
__device__ __forceinline__ T std_max(T a, T b) { return (a < b) ? b : a; }
template <class T>
__device__ __forceinline__ T std_clamp(T v, T lo, T hi) { return (v < lo) ? lo : ((hi < v) ? hi : v); }
__device__ __forceinline__ double dmin(double a, double b) { return std_min(a, b); }
__device__ __forceinline__ double dmax(double a, double b) { return std_max(a, b); }
__device__ __forceinline__ double dclamp(double v, double lo, double hi) { return std_clamp(v, lo, hi); }
namespace f32 {
__device__ __forceinline__ float fmin_std(float a, float b) { return std_min(a, b); }
__device__ __forceinline__ float fmax_std(float a, float b) { return std_max(a, b); }
__device__ __forceinline__ float fclamp_std(float v, float lo, float hi) { return std_clamp(v, lo, hi); }
}  // namespace f32

__device__ __forceinline__ double mt_abs(double v) { return __builtin_fabs(v); }
__device__ __forceinline__ float mt_abs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double mt_sqrt(double v) { return __builtin_sqrt(v); }
__device__ __forceinline__ float mt_sqrt(float v) { return __builtin_sqrtf(v); }
template <class T>
__device__ __forceinline__ T max_abs3(T x, T y, T z) {  // more_thuente.h:409-411
  return std_max(mt_abs(x), std_max(mt_abs(y), mt_abs(z)));
}

// Interval state updated by cstep (all by value: keeps everything in registers).
template <class T>
struct MtInterval {
  T stx, fx, dx;  // best step so far, its value and derivative
  T sty, fy, dy;  // other end of the interval of uncertainty
  T stp;          // current / next trial step
  bool brackt;
  int info;
  int rc;         // cstep's return value (0, or -1 on invalid input)
};

// more_thuente.h:261-407 in the reference's own control flow (a wavefront's segments rarely need different cases in
// the same call; an operand-select form that issues the arithmetic once measured 1 % slower on every workload,
// profiles/r2_ab_cstep_select.txt).  fp, dp are the value/derivative at the trial stp;
// stpmin/stpmax are the bracket bounds computed by cvsrch.  rc = 0, or -1 on
// invalid input (info = 0, nothing else changed).
template <class T>
__device__ __forceinline__ MtInterval<T> mt_cstep(MtInterval<T> in, const T fp, const T dp, const T stpmin,
                                                  const T stpmax) {
  constexpr T zero = static_cast<T>(0.0), two = static_cast<T>(2.0), three = static_cast<T>(3.0);
  T stx = in.stx, fx = in.fx, dx = in.dx, sty = in.sty, fy = in.fy, dy = in.dy, stp = in.stp;
  bool brackt = in.brackt;
  int info;
  info = 0;
  bool bound = false;
  if ((brackt && ((stp <= std_min(stx, sty)) || (stp >= std_max(stx, sty)))) ||
      (dx * (stp - stx) >= zero) || (stpmax < stpmin)) {
    in.info = 0;
    in.rc = -1;
    return in;
  }
  const T sgnd = dp * (dx / mt_abs(dx));
  T stpf = zero, stpc = zero, stpq = zero;
  if (fp > fx) {  // Case 1: higher function value -> minimum is bracketed.
    info = 1;
    bound = true;
    const T theta = three * (fx - fp) / (stp - stx) + dx + dp;
    const T s = max_abs3(theta, dx, dp);
    T gamma = s * mt_sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp < stx) gamma = -gamma;
    const T p = (gamma - dx) + theta;
    const T q = ((gamma - dx) + gamma) + dp;
    const T r = p / q;
    stpc = stx + r * (stp - stx);
    stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / two) * (stp - stx);
    if (mt_abs(stpc - stx) < mt_abs(stpq - stx))
      stpf = stpc;
    else
      stpf = stpc + (stpq - stpc) / two;
    brackt = true;
  } else if (sgnd < zero) {  // Case 2: derivatives change sign -> bracketed.
    info = 2;
    bound = false;
    const T theta = three * (fx - fp) / (stp - stx) + dx + dp;
    const T s = max_abs3(theta, dx, dp);
    T gamma = s * mt_sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp > stx) gamma = -gamma;
    const T p = (gamma - dp) + theta;
    const T q = ((gamma - dp) + gamma) + dx;
    const T r = p / q;
    stpc = stp + r * (stx - stp);
    stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (mt_abs(stpc - stp) > mt_abs(stpq - stp))
      stpf = stpc;
    else
      stpf = stpq;
    brackt = true;
  } else if (mt_abs(dp) < mt_abs(dx)) {  // Case 3: |derivative| decreases.
    info = 3;
    bound = true;
    const T theta = three * (fx - fp) / (stp - stx) + dx + dp;
    const T s = max_abs3(theta, dx, dp);
    T gamma = s * mt_sqrt(std_max(zero, (theta / s) * (theta / s) - (dx / s) * (dp / s)));
    if (stp > stx) gamma = -gamma;
    const T p = (gamma - dp) + theta;
    const T q = (gamma + (dx - dp)) + gamma;
    const T r = p / q;
    if ((r < zero) & (gamma != zero)) {
      stpc = stp + r * (stx - stp);
    } else if (stp > stx) {
      stpc = stpmax;
    } else {
      stpc = stpmin;
    }
    stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (brackt) {
      stpf = (mt_abs(stp - stpc) < mt_abs(stp - stpq)) ? stpc : stpq;
    } else {
      stpf = (mt_abs(stp - stpc) > mt_abs(stp - stpq)) ? stpc : stpq;
    }
  } else {  // Case 4: |derivative| does not decrease.
    info = 4;
    bound = false;
    if (brackt) {
      const T theta = three * (fp - fy) / (sty - stp) + dy + dp;
      const T s = max_abs3(theta, dy, dp);
      T gamma = s * mt_sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s));
      if (stp > sty) gamma = -gamma;
      const T p = (gamma - dp) + theta;
      const T q = ((gamma - dp) + gamma) + dy;
      const T r = p / q;
      stpc = stp + r * (sty - stp);
      stpf = stpc;
    } else if (stp > stx) {
      stpf = stpmax;
    } else {
      stpf = stpmin;
    }
  }
  // Update the interval of uncertainty.
  if (fp > fx) {
    sty = stp;
    fy = fp;
    dy = dp;
  } else {
    if (sgnd < zero) {
      sty = stx;
      fy = fx;
      dy = dx;
    }
    stx = stp;
    fx = fp;
    dx = dp;
  }
  stpf = std_clamp(stpf, stpmin, stpmax);
  stp = stpf;
  if (brackt & bound) {
    if (sty > stx) {
      stp = std_min(stx + static_cast<T>(0.66) * (sty - stx), stp);
    } else {
      stp = std_max(stx + static_cast<T>(0.66) * (sty - stx), stp);
    }
  }
  MtInterval<T> out;
  out.stx = stx; out.fx = fx; out.dx = dx;
  out.sty = sty; out.fy = fy; out.dy = dy;
  out.stp = stp;
  out.brackt = brackt;
  out.info = info;
  out.rc = 0;
  return out;
}

// One search between two of its evaluations: cvsrch (:137-256) cut at its objective evaluation.  The 17 fields are
// those the ask/tell kernels' Scalars keep under the same names (the flags as int32_t); stmin / stmax are among them
// because without a bracket stmax is formed from the step BEFORE the clamp and the `stp = stx` fallback, so it cannot
// be re-formed from the step that was evaluated.
//   start(); do { evaluate at stp; } while (after_evaluation() == 0);   then stp is the accepted step.
template <class T>
struct MtSearch {
  // more_thuente.h:140-147
  static constexpr T xtol = static_cast<T>(1e-15), ftol = static_cast<T>(1e-4), gtol = static_cast<T>(0.9);
  static constexpr T stpmin = static_cast<T>(1e-15), stpmax = static_cast<T>(1e15), xtrapf = static_cast<T>(4.0);
  static constexpr int maxfev = 20;

  // (not initialised: every read follows load() or start(), which set all 17)
  T stx, fx, dgx, sty, fy, dgy, stp;
  T width, width1, finit, dginit, stmin, stmax;
  bool brackt, stage1;
  int infoc, ls_nfev;

  template <class Scalars>
  __device__ __forceinline__ void load(const Scalars* sc) {
    stx = sc->stx; fx = sc->fx; dgx = sc->dgx;
    sty = sc->sty; fy = sc->fy; dgy = sc->dgy;
    stp = sc->stp; width = sc->width; width1 = sc->width1;
    finit = sc->finit; dginit = sc->dginit; stmin = sc->stmin; stmax = sc->stmax;
    brackt = sc->brackt != 0; stage1 = sc->stage1 != 0; infoc = sc->infoc; ls_nfev = sc->ls_nfev;
  }
  template <class Scalars>
  __device__ __forceinline__ void store(Scalars* sc) const {
    sc->stx = stx; sc->fx = fx; sc->dgx = dgx;
    sc->sty = sty; sc->fy = fy; sc->dgy = dgy;
    sc->stp = stp; sc->width = width; sc->width1 = width1;
    sc->finit = finit; sc->dginit = dginit; sc->stmin = stmin; sc->stmax = stmax;
    sc->brackt = brackt; sc->stage1 = stage1; sc->infoc = infoc; sc->ls_nfev = ls_nfev;
  }

  // more_thuente.h:158-177: a search from value f and directional derivative dg0 = g.s < 0 (the caller has taken the
  // dg0 >= 0 return of :152-156 itself) with the first step stp0; leaves the first trial step in stp
  __device__ __forceinline__ void start(T f, T dg0, T stp0) {
    brackt = false;
    stage1 = true;
    infoc = 1;
    ls_nfev = 0;
    finit = f;
    dginit = dg0;
    width = stpmax - stpmin;
    width1 = static_cast<T>(2.0) * width;
    stx = static_cast<T>(0.0); fx = finit; dgx = dginit;
    sty = static_cast<T>(0.0); fy = finit; dgy = dginit;
    stp = stp0;
    before_evaluation();
  }

  // more_thuente.h:179-195: the interval, the clamp and the fallback before an evaluation
  __device__ __forceinline__ void before_evaluation() {
    if (brackt) {
      stmin = std_min(stx, sty);
      stmax = std_max(stx, sty);
    } else {
      stmin = stx;
      stmax = stp + xtrapf * (stp - stx);
    }
    stp = std_clamp(stp, stpmin, stpmax);
    if ((brackt && ((stp <= stmin) || (stp >= stmax))) || (ls_nfev >= maxfev - 1) || (infoc == 0) ||
        (brackt && ((stmax - stmin) <= (xtol * stmax)))) {
      stp = stx;
    }
  }

  // more_thuente.h:200-252: the loop body after the evaluation at stp gave the value f.  dg_of(): the path's directional
  // derivative dg = g.s (and its count of the evaluation), called where cvsrch takes it (:200-201), after dgtest and the
  // search's own count — the fp64 Lbfgs step kernel ran 2.4 % longer with the segment reduction ahead of these
  // (profiles/ask_tell_refactor_ab.txt, section 1).  Returns
  // cvsrch's info: != 0, the search has ended and stp is the accepted step; 0, the search goes on and stp is the next
  // trial step, before_evaluation() applied.
  template <class DirectionalDerivative>
  __device__ __forceinline__ int after_evaluation(T f, DirectionalDerivative dg_of) {
    const T dgtest = ftol * dginit;
    ls_nfev++;
    const T dg = dg_of();
    const T ftest1 = finit + stp * dgtest;
    int info = 0;
    if ((brackt & ((stp <= stmin) | (stp >= stmax))) | (infoc == 0)) info = 6;
    if ((stp == stpmax) & (f <= ftest1) & (dg <= dgtest)) info = 5;
    if ((stp == stpmin) & ((f > ftest1) | (dg >= dgtest))) info = 4;
    if (ls_nfev >= maxfev) info = 3;
    if (brackt & (stmax - stmin <= xtol * stmax)) info = 2;
    if ((f <= ftest1) & (mt_abs(dg) <= gtol * (-dginit))) info = 1;
    if (info != 0) return info;
    if (stage1 & (f <= ftest1) & (dg >= std_min(ftol, gtol) * dginit)) stage1 = false;
    // :225-244: cstep on the modified function while stage 1 lasts and the value is lower but not low enough, on f
    // itself otherwise
    const bool modified = stage1 & (f <= fx) & (f > ftest1);
    MtInterval<T> iv{};
    iv.stx = stx; iv.sty = sty; iv.stp = stp; iv.brackt = brackt; iv.info = infoc;
    iv.fx = modified ? fx - stx * dgtest : fx;
    iv.fy = modified ? fy - sty * dgtest : fy;
    iv.dx = modified ? dgx - dgtest : dgx;
    iv.dy = modified ? dgy - dgtest : dgy;
    const T fm = modified ? f - stp * dgtest : f;
    const T dgm = modified ? dg - dgtest : dg;
    iv = mt_cstep(iv, fm, dgm, stmin, stmax);
    stx = iv.stx; sty = iv.sty; stp = iv.stp; brackt = iv.brackt; infoc = iv.info;
    fx = modified ? iv.fx + stx * dgtest : iv.fx;
    fy = modified ? iv.fy + sty * dgtest : iv.fy;
    dgx = modified ? iv.dx + dgtest : iv.dx;
    dgy = modified ? iv.dy + dgtest : iv.dy;
    if (brackt) {  // :246-252
      if (mt_abs(sty - stx) >= static_cast<T>(0.66) * width1) stp = stx + static_cast<T>(0.5) * (sty - stx);
      width1 = width;
      width = mt_abs(sty - stx);
    }
    before_evaluation();
    return 0;
  }
};

// Profiling build (-DMI355_LBFGS_PHASE_TIMING): the caller's phase clock, so that the trials after the first are charged
// to a phase of their own (scripts/lbfgs_phases.py).  Nothing of it exists in any other build.
// The kernel reports the clock of lane 0 of each wavefront, so the switch must be taken by lane 0 whenever ANY segment
// of the wavefront goes on to a later trial — also when lane 0's own segment is done and only waits for the others.
// It therefore stands where every segment that ran the first trial is still active (before the divergent exit), under
// a ballot of "this segment continues".  (A segment that returned at once, dginit >= 0, is not there; if it is segment
// 0 the later trials of that pass stay charged to the first-trial phase.  That does not occur on the flagship batches.)
#ifdef MI355_LBFGS_PHASE_TIMING
struct MtPhaseClock {
  unsigned long long* cycles;
  unsigned long long* t0;
  int* cur;
};
#define MI355_MT_PHASE_PARAM , const MtPhaseClock* phase_clock = nullptr
#define MI355_MT_PHASE_LATER_IF_ANY(continues)                        \
  do {                                                                \
    if (phase_clock != nullptr && __builtin_amdgcn_ballot_w64(continues) != 0) { \
      const unsigned long long now_ = __builtin_readcyclecounter();   \
      phase_clock->cycles[*phase_clock->cur] += now_ - *phase_clock->t0; \
      *phase_clock->t0 = now_;                                        \
      *phase_clock->cur = 11;                                         \
    }                                                                 \
  } while (0)
#else
#define MI355_MT_PHASE_PARAM
#define MI355_MT_PHASE_LATER_IF_ANY(continues) do { } while (0)
#endif

// more_thuente.h:137-256 with the State-overload prologue of :120-135.
// In:  x = start point, f/g = value/gradient there, d = NEGATED search direction
//      (the line search runs along s = -d, lbfgs.h:231-232), stp = initial step,
//      dginit = g.s.   Out: x, f, g at the last evaluated trial.
// Working with d instead of a separate s = -d saves E register pairs and is exact:
// wa + stp*(-d) == wa - stp*d and g.(-d) == -(g.d) bit for bit (negation commutes
// with IEEE rounding).
// Returns the number of objective evaluations performed.
template <int W, int E, class Obj, class AR = ArithExact>
__device__ __forceinline__ int mt_cvsrch(const Obj& obj, double (&x)[E], double& f, double (&g)[E],
                                         double stp, const double (&d)[E], const double dginit,
                                         int n, int sl MI355_MT_PHASE_PARAM) {
  int info = 0;
  int infoc = 1;
  using S = MtSearch<double>;
  constexpr double xtol = S::xtol, ftol = S::ftol, gtol = S::gtol, stpmin = S::stpmin, stpmax = S::stpmax;
  constexpr int maxfev = S::maxfev;
  int nfev = 0;

  // dginit = g.s (:151) is supplied by the caller, which already holds it.
  if (dginit >= 0.0) return 0;  // no descent direction: x, f, g untouched (:152-156)

  bool brackt = false;
  bool stage1 = true;
  const double finit = f;
  const double dgtest = ftol * dginit;
  double width = stpmax - stpmin;
  double width1 = 2.0 * width;
  double wa[E];
#pragma unroll
  for (int e = 0; e < E; ++e) wa[e] = x[e];

  double stx = 0.0, fx = finit, dgx = dginit;
  double sty = 0.0, fy = finit, dgy = dginit;
  double stmin, stmax;

  while (true) {
    if (brackt) {
      stmin = dmin(stx, sty);
      stmax = dmax(stx, sty);
    } else {
      stmin = stx;
      stmax = stp + S::xtrapf * (stp - stx);
    }
    stp = dclamp(stp, stpmin, stpmax);
    if ((brackt && ((stp <= stmin) || (stp >= stmax))) || (nfev >= maxfev - 1) || (infoc == 0) ||
        (brackt && ((stmax - stmin) <= (xtol * stmax)))) {
      stp = stx;
    }
    {
      // The trial point lives only for the evaluation; the accepted one is re-formed after
      // the loop.  That keeps E doubles per lane out of the step-selection arithmetic below,
      // which is where the kernel's register budget (waves per SIMD) is set.
      double xt[E];
#pragma unroll
      for (int e = 0; e < E; ++e) xt[e] = AR::nmadd(stp, d[e], wa[e]);  // wa + stp * s
      f = obj_eval<W, E, AR>(obj, xt, g, n, sl);
    }
    nfev++;
    const double dg = -seg_dot<W, E, AR>(g, d);  // g.s
    const double ftest1 = finit + stp * dgtest;

    if ((brackt & ((stp <= stmin) | (stp >= stmax))) | (infoc == 0)) info = 6;
    if ((stp == stpmax) & (f <= ftest1) & (dg <= dgtest)) info = 5;
    if ((stp == stpmin) & ((f > ftest1) | (dg >= dgtest))) info = 4;
    if (nfev >= maxfev) info = 3;
    if (brackt & (stmax - stmin <= xtol * stmax)) info = 2;
    if ((f <= ftest1) & (__builtin_fabs(dg) <= gtol * (-dginit))) info = 1;
    MI355_MT_PHASE_LATER_IF_ANY(info == 0);
    if (info != 0) break;

    if (stage1 & (f <= ftest1) & (dg >= dmin(ftol, gtol) * dginit)) stage1 = false;

    // :225-244.  During stage 1 the step is computed on the modified function
    // psi(a) = f(a) - f(0) - a*dgtest; both branches call the same cstep, so
    // the arguments are selected first and cstep is instantiated once.
    const bool modified = stage1 & (f <= fx) & (f > ftest1);
    MtInterval<double> iv;
    iv.stx = stx; iv.sty = sty; iv.stp = stp; iv.brackt = brackt; iv.info = infoc; iv.rc = 0;
    iv.fx = modified ? fx - stx * dgtest : fx;
    iv.fy = modified ? fy - sty * dgtest : fy;
    iv.dx = modified ? dgx - dgtest : dgx;
    iv.dy = modified ? dgy - dgtest : dgy;
    const double fm = modified ? f - stp * dgtest : f;
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
  }
  // the accepted point, re-formed from the accepted step: same operands, same bits
#pragma unroll
  for (int e = 0; e < E; ++e) x[e] = AR::nmadd(stp, d[e], wa[e]);
  return nfev;
}

// The same search for the lean solve kernels (OPT::kFixed, lbfgs_kernel.hpp): the first trial peeled out of the loop.
// Four line searches in five end at their first trial, and the segments of a wavefront run a search loop until the
// last of them has left it, so the general trip — written for any (brackt, stx, nfev, infoc) — would be what every
// segment pays every iteration.  In the first trip brackt = false, stx = sty = 0, ls_nfev = 0 and infoc = 1 are
// compile-time constants once start() and after_evaluation() are inlined, so the compiler folds what they decide:
//   stmin = stx = 0 and stmax = stp + xtrapf * (stp - 0) (stp - 0.0 is stp, bit for bit, for every stp);
//   the `stp = stx` fallback and info 6 / 3 / 2 cannot fire (no bracket, nfev = 1 < maxfev, infoc = 1);
//   info 5, 4, 1 are tested in the reference's order (a later test overwrites an earlier one).
// Segments with info == 0 go on to the loop, which sits under one branch that a wavefront skips when none of its
// segments continues.  (The profiling hook stands after the first after_evaluation(): the first step computation of a
// continuing segment is charged to the first-trial phase.)
// wa: the start point (the caller's copy of x that it keeps for s = x+ - x; x itself is only written at the end).
template <int W, int E, class Obj, class AR = ArithExact>
__device__ __forceinline__ int mt_cvsrch_peeled(const Obj& obj, double (&x)[E], double& f, double (&g)[E],
                                                double stp, const double (&d)[E], const double dginit,
                                                const double (&wa)[E], int n, int sl MI355_MT_PHASE_PARAM) {
  if (dginit >= 0.0) return 0;  // no descent direction: x, f, g untouched (:152-156)
  MtSearch<double> mt;
  mt.start(f, dginit, stp);
  const auto dg_of = [&] { return -seg_dot<W, E, AR>(g, d); };  // g.s
  {
    double xt[E];
#pragma unroll
    for (int e = 0; e < E; ++e) xt[e] = AR::nmadd(mt.stp, d[e], wa[e]);  // wa + stp * s
    f = obj_eval<W, E, AR>(obj, xt, g, n, sl);
  }
  int info = mt.after_evaluation(f, dg_of);
  MI355_MT_PHASE_LATER_IF_ANY(info == 0);
  if (info == 0) {
    do {
      double xt[E];
#pragma unroll
      for (int e = 0; e < E; ++e) xt[e] = AR::nmadd(mt.stp, d[e], wa[e]);  // wa + stp * s
      f = obj_eval<W, E, AR>(obj, xt, g, n, sl);
      info = mt.after_evaluation(f, dg_of);
    } while (info == 0);
  }
  // the accepted point, re-formed from the accepted step: same operands, same bits
#pragma unroll
  for (int e = 0; e < E; ++e) x[e] = AR::nmadd(mt.stp, d[e], wa[e]);
  return mt.ls_nfev;
}

namespace f32 {

// mt_cvsrch on a float function.  Kept from the fp64 routine: dginit >= 0 returns with x, f, g untouched; d is the
// NEGATED search direction; the accepted point is re-formed from the accepted step.
template <int W, int E, class Obj>
__device__ __forceinline__ int mt_cvsrch(const Obj& obj, float (&x)[E], float& f, float (&g)[E], float stp,
                                         const float (&d)[E], const float dginit, int n, int sl) {
  int info = 0;
  int infoc = 1;
  using S = MtSearch<float>;
  const float xtol = S::xtol, ftol = S::ftol, gtol = S::gtol, stpmin = S::stpmin, stpmax = S::stpmax;
  constexpr int maxfev = S::maxfev;
  int nfev = 0;

  if (dginit >= static_cast<float>(0)) return 0;  // no descent direction: x, f, g untouched (:152-156)

  bool brackt = false;
  bool stage1 = true;
  const float finit = f;
  const float dgtest = ftol * dginit;
  float width = stpmax - stpmin;
  float width1 = static_cast<float>(2) * width;
  float wa[E];
#pragma unroll
  for (int e = 0; e < E; ++e) wa[e] = x[e];

  float stx = static_cast<float>(0), fx = finit, dgx = dginit;
  float sty = static_cast<float>(0), fy = finit, dgy = dginit;
  float stmin, stmax;

  while (true) {
    if (brackt) {
      stmin = fmin_std(stx, sty);
      stmax = fmax_std(stx, sty);
    } else {
      stmin = stx;
      stmax = stp + S::xtrapf * (stp - stx);
    }
    stp = fclamp_std(stp, stpmin, stpmax);
    if ((brackt && ((stp <= stmin) || (stp >= stmax))) || (nfev >= maxfev - 1) || (infoc == 0) ||
        (brackt && ((stmax - stmin) <= (xtol * stmax)))) {
      stp = stx;
    }
    {
      float xt[E];
#pragma unroll
      for (int e = 0; e < E; ++e) xt[e] = wa[e] - stp * d[e];  // wa + stp * s
      f = obj.template eval<W, E>(xt, g, n, sl);
    }
    nfev++;
    const float dg = -seg_dot<W, E>(g, d);  // g.s
    const float ftest1 = finit + stp * dgtest;

    if ((brackt & ((stp <= stmin) | (stp >= stmax))) | (infoc == 0)) info = 6;
    if ((stp == stpmax) & (f <= ftest1) & (dg <= dgtest)) info = 5;
    if ((stp == stpmin) & ((f > ftest1) | (dg >= dgtest))) info = 4;
    if (nfev >= maxfev) info = 3;
    if (brackt & (stmax - stmin <= xtol * stmax)) info = 2;
    if ((f <= ftest1) & (__builtin_fabsf(dg) <= gtol * (-dginit))) info = 1;
    if (info != 0) break;

    if (stage1 & (f <= ftest1) & (dg >= fmin_std(ftol, gtol) * dginit)) stage1 = false;

    // :225-244: during stage 1 the step is computed on the modified function; both branches call the same cstep
    const bool modified = stage1 & (f <= fx) & (f > ftest1);
    MtInterval<float> iv;
    iv.stx = stx; iv.sty = sty; iv.stp = stp; iv.brackt = brackt; iv.info = infoc; iv.rc = 0;
    iv.fx = modified ? fx - stx * dgtest : fx;
    iv.fy = modified ? fy - sty * dgtest : fy;
    iv.dx = modified ? dgx - dgtest : dgx;
    iv.dy = modified ? dgy - dgtest : dgy;
    const float fm = modified ? f - stp * dgtest : f;
    const float dgm = modified ? dg - dgtest : dg;
    iv = mt_cstep(iv, fm, dgm, stmin, stmax);
    stx = iv.stx; sty = iv.sty; stp = iv.stp; brackt = iv.brackt; infoc = iv.info;
    fx = modified ? iv.fx + stx * dgtest : iv.fx;
    fy = modified ? iv.fy + sty * dgtest : iv.fy;
    dgx = modified ? iv.dx + dgtest : iv.dx;
    dgy = modified ? iv.dy + dgtest : iv.dy;
    if (brackt) {
      if (__builtin_fabsf(sty - stx) >= static_cast<float>(0.66) * width1) stp = stx + static_cast<float>(0.5) * (sty - stx);
      width1 = width;
      width = __builtin_fabsf(sty - stx);
    }
  }
  // the accepted point, re-formed from the accepted step: same operands, same bits
#pragma unroll
  for (int e = 0; e < E; ++e) x[e] = wa[e] - stp * d[e];
  return nfev;
}

}  // namespace f32
}  // namespace mi355
