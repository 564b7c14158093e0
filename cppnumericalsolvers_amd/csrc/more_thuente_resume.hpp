// more_thuente_resume.hpp — MoreThuente::cvsrch (linesearch/more_thuente.h:137-256) cut at its objective evaluation: the
// scalar state of one search and the two halves of the loop body around the evaluation, for the kernels that hand the
// evaluation to the caller (lbfgs_ask_tell_kernel.hpp, lbfgs_ask_tell_f32_kernel.hpp, lbfgsb_ask_tell_kernel.hpp).
//
// The statements are those of the persistent searches — mt_cvsrch of more_thuente_device.hpp for double, of
// more_thuente_f32_device.hpp for float — on the same operands in the same order, so a caller that evaluates with the
// library's own functor reproduces the persistent kernels bit for bit.  Every constant is static_cast<T>(double
// literal), the double literal rounded once, as the reference forms ScalarType(1e-4); the float unit is built with
// -ffp-contract=off and relies on the operand order of every expression below.  Everything here is segment-uniform:
// every lane of a segment carries the same values and takes the same branches.
//
// What stays with the kernels, because it differs per path: counting the evaluation (nfev) and the directional
// derivative dg = g.s (handed to after_evaluation() as a callable), forming the trial point from stp, and the phase word.
#pragma once
#include "more_thuente_device.hpp"
#include "more_thuente_f32_device.hpp"

namespace mi355 {

// the names a scalar type brings to the search: std::min / max / clamp / fabs as its persistent search spells them,
// the interval cstep works on, and cstep itself
template <class T>
struct MtScalar;

template <>
struct MtScalar<double> {
  using Interval = StepInterval;
  __device__ __forceinline__ static double min(double a, double b) { return dmin(a, b); }
  __device__ __forceinline__ static double max(double a, double b) { return dmax(a, b); }
  __device__ __forceinline__ static double clamp(double v, double lo, double hi) { return dclamp(v, lo, hi); }
  __device__ __forceinline__ static double abs(double v) { return __builtin_fabs(v); }
  __device__ __forceinline__ static Interval cstep(Interval iv, double fp, double dp, double stmin, double stmax) {
    return mt_cstep(iv, fp, dp, stmin, stmax);
  }
};

template <>
struct MtScalar<float> {
  using Interval = f32::StepInterval;
  __device__ __forceinline__ static float min(float a, float b) { return f32::fmin_std(a, b); }
  __device__ __forceinline__ static float max(float a, float b) { return f32::fmax_std(a, b); }
  __device__ __forceinline__ static float clamp(float v, float lo, float hi) { return f32::fclamp_std(v, lo, hi); }
  __device__ __forceinline__ static float abs(float v) { return __builtin_fabsf(v); }
  __device__ __forceinline__ static Interval cstep(Interval iv, float fp, float dp, float stmin, float stmax) {
    return f32::mt_cstep(iv, fp, dp, stmin, stmax);
  }
};

// One search between two of its evaluations.  The 17 fields are those every path's Scalars keeps under the same names
// (the flags as int32_t); stmin / stmax are among them because without a bracket stmax is formed from the step BEFORE
// the clamp and the `stp = stx` fallback, so it cannot be re-formed from the step that was evaluated.
template <class T>
struct MtSearch {
  using S = MtScalar<T>;
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
      stmin = S::min(stx, sty);
      stmax = S::max(stx, sty);
    } else {
      stmin = stx;
      stmax = stp + xtrapf * (stp - stx);
    }
    stp = S::clamp(stp, stpmin, stpmax);
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
    if ((f <= ftest1) & (S::abs(dg) <= gtol * (-dginit))) info = 1;
    if (info != 0) return info;
    if (stage1 & (f <= ftest1) & (dg >= S::min(ftol, gtol) * dginit)) stage1 = false;
    // :225-244: cstep on the modified function while stage 1 lasts and the value is lower but not low enough, on f
    // itself otherwise
    const bool modified = stage1 & (f <= fx) & (f > ftest1);
    typename S::Interval iv{};
    iv.stx = stx; iv.sty = sty; iv.stp = stp; iv.brackt = brackt; iv.info = infoc;
    iv.fx = modified ? fx - stx * dgtest : fx;
    iv.fy = modified ? fy - sty * dgtest : fy;
    iv.dx = modified ? dgx - dgtest : dgx;
    iv.dy = modified ? dgy - dgtest : dgy;
    const T fm = modified ? f - stp * dgtest : f;
    const T dgm = modified ? dg - dgtest : dg;
    iv = S::cstep(iv, fm, dgm, stmin, stmax);
    stx = iv.stx; sty = iv.sty; stp = iv.stp; brackt = iv.brackt; infoc = iv.info;
    fx = modified ? iv.fx + stx * dgtest : iv.fx;
    fy = modified ? iv.fy + sty * dgtest : iv.fy;
    dgx = modified ? iv.dx + dgtest : iv.dx;
    dgy = modified ? iv.dy + dgtest : iv.dy;
    if (brackt) {  // :246-252
      if (S::abs(sty - stx) >= static_cast<T>(0.66) * width1) stp = stx + static_cast<T>(0.5) * (sty - stx);
      width1 = width;
      width = S::abs(sty - stx);
    }
    before_evaluation();
    return 0;
  }
};

}  // namespace mi355
