// more_thuente_f32_device.hpp — Moré–Thuente line search on a wavefront segment, ScalarType = float.
//
// Float counterpart of more_thuente_device.hpp, i.e. of the reference's linesearch/more_thuente.h instantiated on a float
// function: cvsrch :137-256 (with the State-overload prologue :120-135) and cstep :261-407.  Every constant is formed the
// way the reference forms it — ScalarType(1e-4) is static_cast<float>(1e-4), the double literal rounded once — never an
// f-suffixed literal.  Kept from the fp64 routine: dginit >= 0 returns with x, f, g untouched; the "return to best" rule
// (stp = stx) ; the order of the info tests (a later test overwrites an earlier one); the accepted point re-formed from
// the accepted step.  Step-length bookkeeping is scalar and segment-uniform.
#pragma once
#include "wave_primitives_f32.hpp"

namespace mi355 {
namespace f32 {

__device__ __forceinline__ float fmin_std(float a, float b) { return (b < a) ? b : a; }   // std::min
__device__ __forceinline__ float fmax_std(float a, float b) { return (a < b) ? b : a; }   // std::max
__device__ __forceinline__ float fclamp_std(float v, float lo, float hi) {                // std::clamp
  return (v < lo) ? lo : ((hi < v) ? hi : v);
}
__device__ __forceinline__ float max_abs3(float x, float y, float z) {  // more_thuente.h:409-411
  return fmax_std(__builtin_fabsf(x), fmax_std(__builtin_fabsf(y), __builtin_fabsf(z)));
}

struct StepInterval {
  float stx, fx, dx;  // best step so far, its value and derivative
  float sty, fy, dy;  // other end of the interval of uncertainty
  float stp;          // current / next trial step
  bool brackt;
  int info;
};

// more_thuente.h:261-407 in the reference's own control flow.  fp, dp: value / derivative at the trial stp; stpmin,
// stpmax: the bounds computed by cvsrch.  Invalid input: info = 0, nothing else changed.
__device__ __forceinline__ StepInterval mt_cstep(StepInterval in, const float fp, const float dp, const float stpmin,
                                                 const float stpmax) {
  float stx = in.stx, fx = in.fx, dx = in.dx, sty = in.sty, fy = in.fy, dy = in.dy, stp = in.stp;
  bool brackt = in.brackt;
  int info = 0;
  bool bound = false;
  const float zero = static_cast<float>(0), two = static_cast<float>(2), three = static_cast<float>(3);
  if ((brackt && ((stp <= fmin_std(stx, sty)) || (stp >= fmax_std(stx, sty)))) || (dx * (stp - stx) >= zero) ||
      (stpmax < stpmin)) {
    in.info = 0;
    return in;
  }
  const float sgnd = dp * (dx / __builtin_fabsf(dx));
  float stpf = 0, stpc = 0, stpq = 0;
  if (fp > fx) {  // Case 1
    info = 1;
    bound = true;
    const float theta = three * (fx - fp) / (stp - stx) + dx + dp;
    const float s = max_abs3(theta, dx, dp);
    float gamma = s * __builtin_sqrtf((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp < stx) gamma = -gamma;
    const float p = (gamma - dx) + theta;
    const float q = ((gamma - dx) + gamma) + dp;
    const float r = p / q;
    stpc = stx + r * (stp - stx);
    stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / two) * (stp - stx);
    if (__builtin_fabsf(stpc - stx) < __builtin_fabsf(stpq - stx))
      stpf = stpc;
    else
      stpf = stpc + (stpq - stpc) / two;
    brackt = true;
  } else if (sgnd < zero) {  // Case 2
    info = 2;
    bound = false;
    const float theta = three * (fx - fp) / (stp - stx) + dx + dp;
    const float s = max_abs3(theta, dx, dp);
    float gamma = s * __builtin_sqrtf((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp > stx) gamma = -gamma;
    const float p = (gamma - dp) + theta;
    const float q = ((gamma - dp) + gamma) + dx;
    const float r = p / q;
    stpc = stp + r * (stx - stp);
    stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (__builtin_fabsf(stpc - stp) > __builtin_fabsf(stpq - stp))
      stpf = stpc;
    else
      stpf = stpq;
    brackt = true;
  } else if (__builtin_fabsf(dp) < __builtin_fabsf(dx)) {  // Case 3
    info = 3;
    bound = true;
    const float theta = three * (fx - fp) / (stp - stx) + dx + dp;
    const float s = max_abs3(theta, dx, dp);
    float gamma = s * __builtin_sqrtf(fmax_std(zero, (theta / s) * (theta / s) - (dx / s) * (dp / s)));
    if (stp > stx) gamma = -gamma;
    const float p = (gamma - dp) + theta;
    const float q = (gamma + (dx - dp)) + gamma;
    const float r = p / q;
    if ((r < zero) & (gamma != zero)) {
      stpc = stp + r * (stx - stp);
    } else if (stp > stx) {
      stpc = stpmax;
    } else {
      stpc = stpmin;
    }
    stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (brackt) {
      stpf = (__builtin_fabsf(stp - stpc) < __builtin_fabsf(stp - stpq)) ? stpc : stpq;
    } else {
      stpf = (__builtin_fabsf(stp - stpc) > __builtin_fabsf(stp - stpq)) ? stpc : stpq;
    }
  } else {  // Case 4
    info = 4;
    bound = false;
    if (brackt) {
      const float theta = three * (fp - fy) / (sty - stp) + dy + dp;
      const float s = max_abs3(theta, dy, dp);
      float gamma = s * __builtin_sqrtf((theta / s) * (theta / s) - (dy / s) * (dp / s));
      if (stp > sty) gamma = -gamma;
      const float p = (gamma - dp) + theta;
      const float q = ((gamma - dp) + gamma) + dy;
      const float r = p / q;
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
  stpf = fclamp_std(stpf, stpmin, stpmax);
  stp = stpf;
  if (brackt & bound) {
    const float c66 = static_cast<float>(0.66);
    if (sty > stx) {
      stp = fmin_std(stx + c66 * (sty - stx), stp);
    } else {
      stp = fmax_std(stx + c66 * (sty - stx), stp);
    }
  }
  StepInterval out;
  out.stx = stx; out.fx = fx; out.dx = dx;
  out.sty = sty; out.fy = fy; out.dy = dy;
  out.stp = stp;
  out.brackt = brackt;
  out.info = info;
  return out;
}

// more_thuente.h:137-256.  In: x = start point, f / g = value / gradient there, d = NEGATED search direction (the search
// runs along s = -d: wa + stp * (-d) == wa - stp * d and g.(-d) == -(g.d) bit for bit), stp = initial step, dginit = g.s.
// Out: x, f, g at the last evaluated trial.  Returns the number of objective evaluations.
template <int W, int E, class Obj>
__device__ __forceinline__ int mt_cvsrch(const Obj& obj, float (&x)[E], float& f, float (&g)[E], float stp,
                                         const float (&d)[E], const float dginit, int n, int sl) {
  int info = 0;
  int infoc = 1;
  const float xtol = static_cast<float>(1e-15);
  const float ftol = static_cast<float>(1e-4);
  const float gtol = static_cast<float>(0.9);
  const float stpmin = static_cast<float>(1e-15);
  const float stpmax = static_cast<float>(1e15);
  const float xtrapf = static_cast<float>(4);
  constexpr int maxfev = 20;
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
      stmax = stp + xtrapf * (stp - stx);
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
    StepInterval iv;
    iv.stx = stx; iv.sty = sty; iv.stp = stp; iv.brackt = brackt; iv.info = infoc;
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
