// wave_primitives_f32.hpp — the float counterparts of wave_primitives.hpp's segment reductions (namespace mi355::f32).
//
// The same butterfly: xor1, xor2 quad_perm; xor4 row_half_mirror; xor8 row_mirror; xor16 / xor32 v_permlane{16,32}_swap.
// A float is one register, so a level is ONE 32-bit move and one v_add_f32 / v_max_f32 (fp64: two moves).  Both swap
// levels stay on the VALU: the LDS-crossbar exchange of the fp64 W = 64 butterfly paid because it replaced two swaps
// per level; here it would replace one.
//
// The summation tree is the plain pairwise tree over the zero-padded power-of-two width P = W * E (in-lane pairwise
// first, then the butterfly), the fp64 rule of DESIGN.md section 3: every (W, E) mapping of a problem gives the same bits.
// Max / abs-max follow vmax / vmax_abs / vmax_abs_zero of the fp64 helpers: maxNum semantics (a NaN operand yields the
// other one), |.| as a source modifier, and a fold against 0 so that an all-NaN vector gives 0 — the
// `m = 0; if (m < t) m = t` loop of the reference's lpNorm<Infinity> stand-in and of the CPU twin.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_primitives.hpp"

namespace mi355 {
namespace f32 {

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  // old = 0 + bound_ctrl: lanes whose source is outside the row / wavefront read 0
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// a + partner(a) / max(a, partner(a)) for the two swap levels: the swap leaves {lower copy, upper copy} in the two
// result registers, and both operations are commutative
__device__ __forceinline__ float add_xor16(float v) {
  const unsigned u = static_cast<unsigned>(__float_as_int(v));
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __int_as_float(static_cast<int>(r[0])) + __int_as_float(static_cast<int>(r[1]));
}
__device__ __forceinline__ float add_xor32(float v) {
  const unsigned u = static_cast<unsigned>(__float_as_int(v));
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __int_as_float(static_cast<int>(r[0])) + __int_as_float(static_cast<int>(r[1]));
}
// maxNum of two floats as ONE v_max_f32 (see vmax in wave_primitives.hpp: no signalling NaN arises on this path)
__device__ __forceinline__ float vmax(float a, float b) {
  float r;
  asm("v_max_f32_e64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vmax_abs(float a, float b) {
  float r;
  asm("v_max_f32_e64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vmax_abs_zero(float a) {
  float r;
  asm("v_max_f32_e64 %0, |%1|, 0" : "=v"(r) : "v"(a));
  return r;
}
__device__ __forceinline__ float vmax_zero(float a) {
  float r;
  asm("v_max_f32_e64 %0, %1, 0" : "=v"(r) : "v"(a));
  return r;
}
__device__ __forceinline__ float max_xor16(float v) {
  const unsigned u = static_cast<unsigned>(__float_as_int(v));
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return vmax(__int_as_float(static_cast<int>(r[0])), __int_as_float(static_cast<int>(r[1])));
}
__device__ __forceinline__ float max_xor32(float v) {
  const unsigned u = static_cast<unsigned>(__float_as_int(v));
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return vmax(__int_as_float(static_cast<int>(r[0])), __int_as_float(static_cast<int>(r[1])));
}

// Sum over the W lanes of the caller's segment; result in every lane.
template <int W>
__device__ __forceinline__ float seg_sum(float v) {
  static_assert(W == 1 || W == 2 || W == 4 || W == 8 || W == 16 || W == 32 || W == 64, "W");
  if constexpr (W >= 2) v = v + dpp_mov<kQuadXor1>(v);
  if constexpr (W >= 4) v = v + dpp_mov<kQuadXor2>(v);
  if constexpr (W >= 8) v = v + dpp_mov<kRowHalfMirror>(v);
  if constexpr (W >= 16) v = v + dpp_mov<kRowMirror>(v);
  if constexpr (W >= 32) v = add_xor16(v);
  if constexpr (W >= 64) v = add_xor32(v);
  return v;
}
// Max over the W lanes of the segment (inputs are |.| values folded against 0: never NaN)
template <int W>
__device__ __forceinline__ float seg_max(float v) {
  if constexpr (W >= 2) v = vmax(v, dpp_mov<kQuadXor1>(v));
  if constexpr (W >= 4) v = vmax(v, dpp_mov<kQuadXor2>(v));
  if constexpr (W >= 8) v = vmax(v, dpp_mov<kRowHalfMirror>(v));
  if constexpr (W >= 16) v = vmax(v, dpp_mov<kRowMirror>(v));
  if constexpr (W >= 32) v = max_xor16(v);
  if constexpr (W >= 64) v = max_xor32(v);
  return v;
}

// In-lane pairwise tree over E values (E = 1, 2, 4).
template <int E>
__device__ __forceinline__ float lane_tree_sum(const float (&t)[E]) {
  static_assert(E == 1 || E == 2 || E == 4, "E");
  if constexpr (E == 1) {
    return t[0];
  } else {
    float h[E / 2];
#pragma unroll
    for (int i = 0; i < E / 2; ++i) h[i] = t[2 * i] + t[2 * i + 1];
    return lane_tree_sum<E / 2>(h);
  }
}

// a.b: every product rounded, then the tree (no FMA: the library is built with -ffp-contract=off)
template <int W, int E>
__device__ __forceinline__ float seg_dot(const float (&a)[E], const float (&b)[E]) {
  float t[E];
#pragma unroll
  for (int e = 0; e < E; ++e) t[e] = a[e] * b[e];
  return seg_sum<W>(lane_tree_sum<E>(t));
}

// max |a_j| over the segment, 0 when every coordinate is NaN
template <int W, int E>
__device__ __forceinline__ float seg_amax(const float (&a)[E]) {
  float m;
  if constexpr (E == 1) {
    m = vmax_abs_zero(a[0]);
  } else {
    m = vmax_abs(a[0], a[1]);
#pragma unroll
    for (int e = 2; e + 1 < E; e += 2) m = vmax(m, vmax_abs(a[e], a[e + 1]));
    m = vmax_zero(m);
  }
  return seg_max<W>(m);
}

// Value of `v` in the next / previous lane of the wavefront (lane 63 / lane 0 read 0; callers mask those positions).
__device__ __forceinline__ float from_next_lane(float v) { return dpp_mov<kWaveShl1>(v); }
__device__ __forceinline__ float from_prev_lane(float v) { return dpp_mov<kWaveShr1>(v); }

// Coordinate j of the problem's x on every lane of its segment: the owner contributes x_j, everyone else +0.0
template <int W, int E>
__device__ __forceinline__ float seg_coordinate(const float (&x)[E], int j, int sl) {
  float v = 0.0f;
#pragma unroll
  for (int e = 0; e < E; ++e) v = (sl * E + e == j) ? x[e] : v;
  return seg_sum<W>(v);
}

}  // namespace f32
}  // namespace mi355
