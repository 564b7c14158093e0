// objectives_f32.hpp — the float device functors of the native fp32 L-BFGS path (namespace mi355::f32): Rosenbrock and
// DiagQuadratic with the formulas and the operation order of csrc/objectives.hpp, every operand a float.  Lane `sl` owns
// coordinates j = sl * E + e; coordinates j >= n are padding (x = g = 0).  No FMA (-ffp-contract=off).
#pragma once
#include "wave_primitives_f32.hpp"

namespace mi355 {
namespace f32 {

// f(x) = sum_{i=0}^{n-2} (1 - x_i)^2 + 100 (x_{i+1} - x_i^2)^2
//   t1 = 1 - x_i; t2 = x_{i+1} - x_i x_i; term = t1 t1 + (100 t2) t2
//   g_i = [i + 1 < n] (-2 (1 - x_i) + (200 t2_i) (-2 x_i))  +  [i > 0] 200 t2_{i-1}
struct RosenbrockObjective {
  __device__ __forceinline__ void load(const float*, int, int) {}

  template <int W, int E>
  __device__ __forceinline__ float eval(const float (&x)[E], float (&g)[E], int n, int sl) const {
    const float x_next_lane = from_next_lane(x[0]);
    float t2[E], term[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float xn = (e + 1 < E) ? x[(e + 1 < E) ? e + 1 : e] : x_next_lane;
      const float t1 = 1.0f - x[e];
      t2[e] = xn - x[e] * x[e];
      const float v = t1 * t1 + (100.0f * t2[e]) * t2[e];
      term[e] = (sl * E + e + 1 < n) ? v : 0.0f;
    }
    const float t2_prev_lane = from_prev_lane(t2[E - 1]);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = sl * E + e;
      const bool has_a = j + 1 < n;
      const bool has_b = (j > 0) && (j < n);
      const float a = -2.0f * (1.0f - x[e]) + (200.0f * t2[e]) * (-2.0f * x[e]);
      const float b = 200.0f * ((e > 0) ? t2[(e > 0) ? e - 1 : 0] : t2_prev_lane);
      g[e] = (has_a && has_b) ? (a + b) : (has_a ? a : (has_b ? b : 0.0f));
    }
    return seg_sum<W>(lane_tree_sum<E>(term));
  }
};

// f(x) = sum_i a_i x_i^2 + c: term_i = (a_i x_i) x_i, g_i = (2 a_i) x_i, f = sum + c.  params: n + 1 floats (a, c), each
// the caller's double converted once with static_cast<float> on upload.
template <int E>
struct DiagQuadraticObjective {
  float a_reg[E];
  float c_reg;
  __device__ __forceinline__ void load(const float* params, int n, int sl) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = sl * E + e;
      a_reg[e] = (j < n) ? params[j] : 0.0f;
    }
    c_reg = params[n];
  }
  template <int W, int EE>
  __device__ __forceinline__ float eval(const float (&x)[EE], float (&g)[EE], int n, int sl) const {
    static_assert(EE == E, "E");
    float term[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = sl * E + e;
      term[e] = (j < n) ? (a_reg[e] * x[e]) * x[e] : 0.0f;
      g[e] = (j < n) ? (2.0f * a_reg[e]) * x[e] : 0.0f;
    }
    return seg_sum<W>(lane_tree_sum<E>(term)) + c_reg;
  }
};

}  // namespace f32
}  // namespace mi355
