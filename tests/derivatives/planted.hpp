// planted.hpp — the test functor of the derivative checker (tests/test_gpu_derivatives.py): a correct smooth function whose
// parameter blob can plant ONE error of a given size into its gradient or its Hessian.
//
//     f(x) = sum_i [ 0.5 x_i (Q x)_i + (0.25 c_i) x_i^4 ],   g = Q x + c x^3,   H = Q + 3 diag(c x^2)
//
// Q (n x n, COLUMN MAJOR, symmetric: the generator mirrors it exactly), c (n) and the plant are shared by the batch:
// objective_params holds n n + n + 4 doubles: Q, c, then kind, i, j, size.
//     kind 0   nothing planted
//     kind 1   g_i += size                      (one wrong gradient coordinate)
//     kind 2   H(i, j) += size, H(j, i) += size (one wrong Hessian entry, H stays symmetric; i == j: added once)
//     kind 3   H(i, j) += size                  (planted on one side only: H becomes asymmetric)
// The value is never touched: the finite differences see the correct function.
// Operation order (tests/derivatives/dv_twin.hpp states the same), per coordinate i:
//     sx_i = Q(i, 0) x_0, then sx_i = sx_i + Q(i, j) x_j for j = 1 .. n - 1            (ascending, first term a product)
//     q_i = x_i x_i,   term_i = 0.5 (x_i sx_i) + (0.25 c_i) (q_i q_i),   g_i = sx_i + c_i (q_i x_i)
//     f = the pairwise sum of the terms over the padded width (the in-lane tree, then the segment sum)
//     H(i, i) = Q(i, i) + (3 c_i) q_i
// x_j of another lane comes out of seg_coordinate (exact; a -0.0 arrives as +0.0).
#pragma once

namespace dv_test {

struct Planted {
  static constexpr int kLdsDoubles = 0;
  __host__ __device__ static constexpr int shared_lds_doubles() { return 0; }
  const double* Q;
  const double* c;
  int kind, pi, pj;
  double size;
  __device__ __forceinline__ void load(const double* params, int n, int, double*, double*) {
    Q = params;
    c = params + n * n;
    const double* const plant = params + n * n + n;
    kind = static_cast<int>(plant[0]);
    pi = static_cast<int>(plant[1]);
    pj = static_cast<int>(plant[2]);
    size = plant[3];
  }
  __device__ __forceinline__ void begin_problem(const double*, long long, int, int) {}

  // row sl * E + e of Q x; every lane of the segment takes part in every seg_coordinate, padding lanes keep 0
  template <int W, int E>
  __device__ __forceinline__ void times_q(const double (&x)[E], double (&sx)[E], int n, int sl) const {
#pragma unroll
    for (int e = 0; e < E; ++e) sx[e] = 0.0;
    for (int j = 0; j < n; ++j) {
      const double xj = mi355::seg_coordinate<W, E>(x, j, sl);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = sl * E + e;
        if (i < n) sx[e] = (j == 0) ? Q[i] * xj : sx[e] + Q[j * n + i] * xj;
      }
    }
  }
  template <int W, int E>
  __device__ __forceinline__ double finish(const double (&x)[E], const double (&sx)[E], int n, int sl) const {
    double term[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = sl * E + e;
      const double q = x[e] * x[e];
      term[e] = (i < n) ? 0.5 * (x[e] * sx[e]) + (0.25 * c[i]) * (q * q) : 0.0;
    }
    return mi355::seg_sum<W>(mi355::lane_tree_sum<E>(term));
  }

  template <int W, int E>
  __device__ __forceinline__ double eval(const double (&x)[E], double (&g)[E], int n, int sl) const {
    double sx[E];
    times_q<W, E>(x, sx, n, sl);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = sl * E + e;
      const double q = x[e] * x[e];
      double gi = (i < n) ? sx[e] + c[i] * (q * x[e]) : 0.0;
      if (kind == 1 && i == pi) gi = gi + size;
      g[e] = gi;
    }
    return finish<W, E>(x, sx, n, sl);
  }
  template <int W, int E>
  __device__ __forceinline__ double value(const double (&x)[E], int n, int sl) const {
    double sx[E];
    times_q<W, E>(x, sx, n, sl);
    return finish<W, E>(x, sx, n, sl);
  }
  template <int W, int E>
  __device__ __forceinline__ void hess_full(const double (&x)[E], double* Hm, int n, int sl) const {
    for (int t = sl; t < n * n; t += W) Hm[t] = Q[t];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = sl * E + e;
      if (i < n) Hm[i * n + i] = Q[i * n + i] + (3.0 * c[i]) * (x[e] * x[e]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (sl == 0 && (kind == 2 || kind == 3) && pi >= 0 && pi < n && pj >= 0 && pj < n) {
      Hm[pj * n + pi] = Hm[pj * n + pi] + size;
      if (kind == 2 && pi != pj) Hm[pi * n + pj] = Hm[pi * n + pj] + size;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

}  // namespace dv_test
