// f32_twin.hpp — CPU twin of the native fp32 L-BFGS path (csrc/lbfgs_f32_kernel.hpp): Lbfgs<F, m, MoreThuente> of the
// reference with ScalarType = float (solver/solver.h:181-224, solver/lbfgs.h:72-303, linesearch/more_thuente.h:137-407,
// solver/progress.h:153-327), restated in float with two summation policies:
//   kRefOrder     sequential sums over the n coordinates, the order of the reference over the Eigen stand-in: held bit
//                 for bit to the reference's own headers (tests/lbfgs_f32/ref_harness.cpp);
//   kDeviceOrder  the pairwise tree over the zero-padded width P = W x E of the device mapping, and vectors of length P
//                 whose padding coordinates go through the same element-wise operations as the kernel's padding lanes
//                 (so that the sign of a padding zero is the kernel's): held bit for bit to the device.
// Max-norms are the `m = 0; if (m < t) m = t` fold in both (a NaN is skipped).  Built with -ffp-contract=off: every
// a * b + c is two rounded operations.  Written in float from the start; it shares no code with oracle/.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "common.h"

namespace f32_twin {

enum Order { kRefOrder = 0, kDeviceOrder = 1 };
using Vec = std::vector<float>;

struct Trajectory {  // per-iteration rows and iterates of one solve (null = not recorded)
  int capacity;
  double* rows;  // [capacity][kL32RowWidth]
  float* xs;     // [capacity][n]
  int count;
};

struct Sums {
  Order order;
  int n;      // real coordinates
  int width;  // vector length in device order (W x E); n in reference order
  int length() const { return order == kDeviceOrder ? width : n; }
  // sum of t[0 .. length())
  float sum(Vec t) const {
    if (order == kRefOrder) {
      float s = t[0];
      for (int i = 1; i < n; ++i) s = s + t[i];
      return s;
    }
    for (int len = width; len > 1; len /= 2)
      for (int i = 0; i < len / 2; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    return t[0];
  }
  float dot(const Vec& a, const Vec& b) const {
    Vec t(length());
    for (int i = 0; i < length(); ++i) t[i] = a[i] * b[i];
    return sum(t);
  }
  float amax(const Vec& a) const {
    float m = 0.0f;
    for (int i = 0; i < length(); ++i) {
      const float t = std::abs(a[i]);
      if (m < t) m = t;
    }
    return m;
  }
};

struct Objective {
  int id;
  Vec a;  // DiagQuadratic: a[0 .. n), then c
  // f, and g[0 .. length) (padding: +0)
  float eval(const Sums& s, const Vec& x, Vec& g) const {
    const int n = s.n, L = s.length();
    Vec term(L, 0.0f);
    for (int j = 0; j < L; ++j) g[j] = 0.0f;
    if (id == kL32Rosenbrock) {
      Vec t2(n, 0.0f);
      for (int j = 0; j < n; ++j) {
        const float xn = (j + 1 < n) ? x[j + 1] : 0.0f;
        const float t1 = 1.0f - x[j];
        t2[j] = xn - x[j] * x[j];
        if (j + 1 < n) term[j] = t1 * t1 + (100.0f * t2[j]) * t2[j];
      }
      for (int j = 0; j < n; ++j) {
        const bool has_a = j + 1 < n, has_b = j > 0;
        const float a_ = -2.0f * (1.0f - x[j]) + (200.0f * t2[j]) * (-2.0f * x[j]);
        const float b_ = has_b ? 200.0f * t2[j - 1] : 0.0f;
        g[j] = (has_a && has_b) ? (a_ + b_) : (has_a ? a_ : (has_b ? b_ : 0.0f));
      }
      // the reference-order functor sums the n - 1 terms; the device tree sums all P slots (term[n - 1 ..] = +0)
      if (s.order == kRefOrder) {
        if (n == 1) return 0.0f;
        float f = term[0];
        for (int j = 1; j + 1 < n; ++j) f = f + term[j];
        return f;
      }
      return s.sum(term);
    }
    for (int j = 0; j < n; ++j) {
      term[j] = (a[j] * x[j]) * x[j];
      g[j] = (2.0f * a[j]) * x[j];
    }
    return s.sum(term) + a[n];
  }
};

inline float min_std(float a, float b) { return (b < a) ? b : a; }
inline float max_std(float a, float b) { return (a < b) ? b : a; }
inline float clamp_std(float v, float lo, float hi) { return (v < lo) ? lo : ((hi < v) ? hi : v); }
inline float max_abs3(float x, float y, float z) { return max_std(std::abs(x), max_std(std::abs(y), std::abs(z))); }

// more_thuente.h:261-407
inline void cstep(float& stx, float& fx, float& dx, float& sty, float& fy, float& dy, float& stp, float fp, float dp,
                  bool& brackt, float stpmin, float stpmax, int& info) {
  info = 0;
  bool bound = false;
  const float zero = static_cast<float>(0), two = static_cast<float>(2), three = static_cast<float>(3);
  if ((brackt && ((stp <= min_std(stx, sty)) || (stp >= max_std(stx, sty)))) || (dx * (stp - stx) >= zero) ||
      (stpmax < stpmin))
    return;
  const float sgnd = dp * (dx / std::abs(dx));
  float stpf = 0, stpc = 0, stpq = 0;
  if (fp > fx) {
    info = 1;
    bound = true;
    const float theta = three * (fx - fp) / (stp - stx) + dx + dp;
    const float s = max_abs3(theta, dx, dp);
    float gamma = s * std::sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp < stx) gamma = -gamma;
    const float p = (gamma - dx) + theta;
    const float q = ((gamma - dx) + gamma) + dp;
    const float r = p / q;
    stpc = stx + r * (stp - stx);
    stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / two) * (stp - stx);
    if (std::abs(stpc - stx) < std::abs(stpq - stx))
      stpf = stpc;
    else
      stpf = stpc + (stpq - stpc) / two;
    brackt = true;
  } else if (sgnd < zero) {
    info = 2;
    bound = false;
    const float theta = three * (fx - fp) / (stp - stx) + dx + dp;
    const float s = max_abs3(theta, dx, dp);
    float gamma = s * std::sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp > stx) gamma = -gamma;
    const float p = (gamma - dp) + theta;
    const float q = ((gamma - dp) + gamma) + dx;
    const float r = p / q;
    stpc = stp + r * (stx - stp);
    stpq = stp + (dp / (dp - dx)) * (stx - stp);
    stpf = (std::abs(stpc - stp) > std::abs(stpq - stp)) ? stpc : stpq;
    brackt = true;
  } else if (std::abs(dp) < std::abs(dx)) {
    info = 3;
    bound = true;
    const float theta = three * (fx - fp) / (stp - stx) + dx + dp;
    const float s = max_abs3(theta, dx, dp);
    float gamma = s * std::sqrt(max_std(zero, (theta / s) * (theta / s) - (dx / s) * (dp / s)));
    if (stp > stx) gamma = -gamma;
    const float p = (gamma - dp) + theta;
    const float q = (gamma + (dx - dp)) + gamma;
    const float r = p / q;
    if ((r < zero) & (gamma != zero))
      stpc = stp + r * (stx - stp);
    else if (stp > stx)
      stpc = stpmax;
    else
      stpc = stpmin;
    stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (brackt)
      stpf = (std::abs(stp - stpc) < std::abs(stp - stpq)) ? stpc : stpq;
    else
      stpf = (std::abs(stp - stpc) > std::abs(stp - stpq)) ? stpc : stpq;
  } else {
    info = 4;
    bound = false;
    if (brackt) {
      const float theta = three * (fp - fy) / (sty - stp) + dy + dp;
      const float s = max_abs3(theta, dy, dp);
      float gamma = s * std::sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s));
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
  stpf = clamp_std(stpf, stpmin, stpmax);
  stp = stpf;
  if (brackt & bound) {
    const float c66 = static_cast<float>(0.66);
    if (sty > stx)
      stp = min_std(stx + c66 * (sty - stx), stp);
    else
      stp = max_std(stx + c66 * (sty - stx), stp);
  }
}

// more_thuente.h:137-256 along s = -d (d: the negated search direction, as the kernel carries it); returns the evaluations
inline int cvsrch(const Objective& obj, const Sums& sm, Vec& x, float& f, Vec& g, float stp, const Vec& d, float dginit) {
  const int L = sm.length();
  int info = 0, infoc = 1;
  const float xtol = static_cast<float>(1e-15), ftol = static_cast<float>(1e-4), gtol = static_cast<float>(0.9);
  const float stpmin = static_cast<float>(1e-15), stpmax = static_cast<float>(1e15), xtrapf = static_cast<float>(4);
  const int maxfev = 20;
  int nfev = 0;
  if (dginit >= static_cast<float>(0)) return 0;
  bool brackt = false, stage1 = true;
  const float finit = f;
  const float dgtest = ftol * dginit;
  float width = stpmax - stpmin;
  float width1 = static_cast<float>(2) * width;
  const Vec wa = x;
  float stx = 0, fx = finit, dgx = dginit;
  float sty = 0, fy = finit, dgy = dginit;
  float stmin, stmax;
  while (true) {
    if (brackt) {
      stmin = min_std(stx, sty);
      stmax = max_std(stx, sty);
    } else {
      stmin = stx;
      stmax = stp + xtrapf * (stp - stx);
    }
    stp = clamp_std(stp, stpmin, stpmax);
    if ((brackt && ((stp <= stmin) || (stp >= stmax))) || (nfev >= maxfev - 1) || (infoc == 0) ||
        (brackt && ((stmax - stmin) <= (xtol * stmax))))
      stp = stx;
    for (int j = 0; j < L; ++j) x[j] = wa[j] - stp * d[j];
    f = obj.eval(sm, x, g);
    nfev++;
    const float dg = -sm.dot(g, d);
    const float ftest1 = finit + stp * dgtest;
    if ((brackt & ((stp <= stmin) | (stp >= stmax))) | (infoc == 0)) info = 6;
    if ((stp == stpmax) & (f <= ftest1) & (dg <= dgtest)) info = 5;
    if ((stp == stpmin) & ((f > ftest1) | (dg >= dgtest))) info = 4;
    if (nfev >= maxfev) info = 3;
    if (brackt & (stmax - stmin <= xtol * stmax)) info = 2;
    if ((f <= ftest1) & (std::abs(dg) <= gtol * (-dginit))) info = 1;
    if (info != 0) return nfev;
    if (stage1 & (f <= ftest1) & (dg >= min_std(ftol, gtol) * dginit)) stage1 = false;
    if (stage1 & (f <= fx) & (f > ftest1)) {
      float fm = f - stp * dgtest, fxm = fx - stx * dgtest, fym = fy - sty * dgtest;
      float dgm = dg - dgtest, dgxm = dgx - dgtest, dgym = dgy - dgtest;
      cstep(stx, fxm, dgxm, sty, fym, dgym, stp, fm, dgm, brackt, stmin, stmax, infoc);
      fx = fxm + stx * dgtest;
      fy = fym + sty * dgtest;
      dgx = dgxm + dgtest;
      dgy = dgym + dgtest;
    } else {
      cstep(stx, fx, dgx, sty, fy, dgy, stp, f, dg, brackt, stmin, stmax, infoc);
    }
    if (brackt) {
      if (std::abs(sty - stx) >= static_cast<float>(0.66) * width1) stp = stx + static_cast<float>(0.5) * (sty - stx);
      width1 = width;
      width = std::abs(sty - stx);
    }
  }
}

inline float canonical(float v) { return (v != v) ? std::numeric_limits<float>::quiet_NaN() : v; }
inline double widened(float v) { return (v != v) ? std::numeric_limits<double>::quiet_NaN() : static_cast<double>(v); }

// One solve.  params: DiagQuadratic's n + 1 doubles (null for Rosenbrock).  width: W x E (a power of two >= n), read in
// device order only.
inline void solve_one(int objective, const double* params, int n, int m, Order order, int width, const l32_stop& st,
                      const float* x0, float* x_out, float* f_out, float* g_out, l32_progress* prog,
                      Trajectory* traj = nullptr) {
  const Sums sm{order, n, width};
  const int L = sm.length();
  Objective obj;
  obj.id = objective;
  if (objective == kL32DiagQuadratic) {
    obj.a.resize(n + 1);
    for (int j = 0; j <= n; ++j) obj.a[j] = static_cast<float>(params[j]);
  }
  const float eps = std::numeric_limits<float>::epsilon();
  const float zero = 0.0f, one = 1.0f;
  const float stop_x_delta = static_cast<float>(st.x_delta), stop_f_delta = static_cast<float>(st.f_delta);
  const float stop_gradient_norm = static_cast<float>(st.gradient_norm), stop_past_delta = static_cast<float>(st.past_delta);

  Vec x(L, zero), g(L, zero), d(L), xp(L), gp(L), sv(L), yv(L);
  for (int j = 0; j < n; ++j) x[j] = x0[j];
  std::vector<Vec> S(m, Vec(L)), Y(m, Vec(L));
  Vec sy_mem(m), alpha_mem(m);
  float f = obj.eval(sm, x, g);
  unsigned nfev = 1, sum_k = 0, num_iterations = 0;
  int mem_count = 0, mem_pos = 0;
  float scaling_factor = one;
  int x_delta_violations = 0, f_delta_violations = 0;
  float x_delta = zero, f_delta = zero, gradient_norm = zero;
  int status = -1;
  Vec past_f;
  int past_pos = 0;

  while (true) {
    d = g;
    const int k = mem_count;
    sum_k += k;
    const bool full = mem_count >= m;
    auto slot_of = [&](int i) { return full ? (mem_pos + i) % m : i; };
    for (int i = k - 1; i >= 0; --i) {
      const int slot = slot_of(i);
      const float denom = sy_mem[slot];
      if (std::abs(denom) < eps) continue;
      const float rho = one / denom;
      const float alpha = rho * sm.dot(S[slot], d);
      alpha_mem[i] = alpha;
      for (int j = 0; j < L; ++j) d[j] = d[j] - alpha * Y[slot][j];
    }
    for (int j = 0; j < L; ++j) d[j] = d[j] * scaling_factor;
    for (int i = 0; i < k; ++i) {
      const int slot = slot_of(i);
      const float denom = sy_mem[slot];
      if (std::abs(denom) < eps) continue;
      const float rho = one / denom;
      const float beta = rho * sm.dot(Y[slot], d);
      const float c = alpha_mem[i] - beta;
      for (int j = 0; j < L; ++j) d[j] = d[j] + S[slot][j] * c;
    }
    const float descent_direction = -sm.dot(g, d);
    float dginit = descent_direction;
    float alpha_init = one;
    if (mem_count == 0) {
      const float dn = std::sqrt(sm.dot(d, d));
      alpha_init = (dn > eps) ? one / dn : one;
    }
    const float relative_eps = eps * max_std(one, std::sqrt(sm.dot(x, x)));
    if (!std::isfinite(descent_direction) || descent_direction > -eps * relative_eps) {
      for (int j = 0; j < L; ++j) d[j] = -g[j];
      mem_count = 0;
      mem_pos = 0;
      const float gg = sm.dot(g, g);
      const float gn = std::sqrt(gg);
      alpha_init = (gn > eps) ? one / gn : one;
      dginit = gg;
    }
    xp = x;
    gp = g;
    const float fprev = f;
    nfev += cvsrch(obj, sm, x, f, g, alpha_init, d, dginit);
    if (!std::isfinite(f)) {
      f = fprev;
      x = xp;
      g = gp;
    } else {
      for (int j = 0; j < L; ++j) {
        sv[j] = x[j] - xp[j];
        yv[j] = g[j] - gp[j];
      }
      const float sy = sm.dot(sv, yv);
      const float yy = sm.dot(yv, yv);
      const float sy_threshold = eps * std::sqrt(sm.dot(sv, sv)) * std::sqrt(yy);
      if (sy > sy_threshold) {
        int slot;
        if (mem_count < m) {
          slot = mem_count;
          mem_count++;
        } else {
          slot = mem_pos;
          mem_pos = (mem_pos + 1) % m;
        }
        S[slot] = sv;
        Y[slot] = yv;
        sy_mem[slot] = sy;
      }
      if (yy > eps) {
        const float temp_scaling = sy / yy;
        if (std::isfinite(temp_scaling) && std::abs(temp_scaling) <= static_cast<float>(1e7))
          scaling_factor = max_std(temp_scaling, eps);
      }
    }
    for (int j = n; j < L; ++j) x[j] = zero;

    num_iterations++;
    f_delta = std::abs(f - fprev);
    {
      Vec dx(L);
      for (int j = 0; j < L; ++j) dx[j] = x[j] - xp[j];
      x_delta = sm.amax(dx);
    }
    gradient_norm = sm.amax(g);
    status = 0;
    bool decided = false;
    if ((st.num_iterations > 0) && (num_iterations > st.num_iterations)) {
      status = 1;
      decided = true;
    }
    if (!decided) {
      if ((stop_x_delta > zero) && (x_delta < stop_x_delta)) {
        x_delta_violations++;
        if (x_delta_violations >= st.x_delta_violations) {
          status = 2;
          decided = true;
        }
      } else {
        x_delta_violations = 0;
      }
    }
    if (!decided) {
      const float fscale = st.f_delta_relative ? max_std(max_std(std::abs(f), std::abs(fprev)), one) : one;
      if ((stop_f_delta > zero) && (f_delta < stop_f_delta * fscale)) {
        f_delta_violations++;
        if (f_delta_violations >= st.f_delta_violations) {
          status = 3;
          decided = true;
        }
      } else {
        f_delta_violations = 0;
      }
    }
    if (!decided && st.past > 0) {
      const int p = st.past;
      if (static_cast<int>(past_f.size()) != p) {
        past_f.assign(p, f);
        past_pos = 0;
      }
      if (static_cast<int>(num_iterations) > p) {
        const float pf = past_f[past_pos];
        const float rate = std::abs(pf - f) / max_std(one, std::abs(f));
        if (rate < stop_past_delta) {
          status = 3;
          decided = true;
        }
      }
      if (!decided) {
        past_f[past_pos] = f;
        past_pos = (past_pos + 1) % p;
      }
    }
    if (!decided && stop_gradient_norm > zero) {
      const float scale = st.gradient_norm_relative ? max_std(one, sm.amax(x)) : one;
      if (gradient_norm < stop_gradient_norm * scale) status = 4;
    }
    if (traj != nullptr && traj->count < traj->capacity) {
      double* r = traj->rows + kL32RowWidth * traj->count;
      r[0] = num_iterations;
      r[1] = status;
      r[2] = f;
      r[3] = x_delta;
      r[4] = f_delta;
      r[5] = gradient_norm;
      for (int j = 0; j < n; ++j) traj->xs[traj->count * n + j] = x[j];
      ++traj->count;
    }
    if (status != 0) break;
  }
  for (int j = 0; j < n; ++j) {
    x_out[j] = canonical(x[j]);
    g_out[j] = canonical(g[j]);
  }
  *f_out = canonical(f);
  prog->status = status;
  prog->num_iterations = num_iterations;
  prog->nfev = nfev;
  prog->sum_k = sum_k;
  prog->x_delta = widened(x_delta);
  prog->f_delta = widened(f_delta);
  prog->gradient_norm = widened(gradient_norm);
}

// one evaluation of a row
inline float eval_one(int objective, const double* params, int n, Order order, int width, const float* x_in, float* g_out) {
  const Sums sm{order, n, width};
  Objective obj;
  obj.id = objective;
  if (objective == kL32DiagQuadratic) {
    obj.a.resize(n + 1);
    for (int j = 0; j <= n; ++j) obj.a[j] = static_cast<float>(params[j]);
  }
  Vec x(sm.length(), 0.0f), g(sm.length(), 0.0f);
  for (int j = 0; j < n; ++j) x[j] = x_in[j];
  const float f = obj.eval(sm, x, g);
  for (int j = 0; j < n; ++j) g_out[j] = g[j];
  return f;
}

}  // namespace f32_twin
