// lu_device.hpp — PartialPivLU of one n x n matrix (n <= 64, column major, in the LDS of the problem's segment) and
// the solve of ONE right-hand side against it, spread over the W lanes of the segment.
//
// The order is the one the project pins to (oracle/eigen_shim/Eigen/LU): right-looking elimination, first-maximum pivot
// search from the diagonal down, division by the pivot only when the column's maximum is non-zero; `solve` applies the
// row interchanges in order, then the unit-lower column-oriented substitution, then the upper column-oriented one, which
// divides by lu(j, j) whatever it is.  Every element goes through exactly those operations and neither routine contains
// a reduction, so the bits do not depend on W: a CPU loop in the shim's order gives them too.
//   seg_lu_factor   the element operations of the LU inside seg_hessian_condition (hessian_condition_device.hpp), which
//                   keeps its own copy so that the kernels built on it compile as they did
//   seg_lu_solve    x_i lives in lane i's register; for each column j the lanes read x_j from lane j and L(i, j) / U(i, j)
//                   from LDS, consecutive lanes reading consecutive doubles
#pragma once
#include "wave_primitives.hpp"

namespace mi355 {

constexpr int kLuMaxN = 64;

// LDS doubles of the pivot indices (ints, two per double)
__host__ __device__ inline int lu_pivot_doubles(int n) { return (n + 1) / 2 + 1; }

__device__ __forceinline__ void lu_segment_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// A (n x n, column major) -> its LU in place, piv[k] = the row exchanged with row k
template <int W>
__device__ __forceinline__ void seg_lu_factor(double* A, int* piv, int n, int sl) {
  constexpr int kChunk = 8;
  constexpr int kRows = kLuMaxN / 8;                  // rows of the trailing block a lane may own (W >= 8)
  for (int k = 0; k < n; ++k) {
    double* const colk = A + k * n;
    int p = k;
    double best = __builtin_fabs(colk[k]);
    for (int i0 = k + 1; i0 < n; i0 += kChunk) {      // the first maximum of |column k| from the diagonal down
      double v[kChunk];
#pragma unroll
      for (int u = 0; u < kChunk; ++u) v[u] = __builtin_fabs(colk[(i0 + u < n) ? i0 + u : n - 1]);
#pragma unroll
      for (int u = 0; u < kChunk; ++u)
        if (i0 + u < n && v[u] > best) {
          best = v[u];
          p = i0 + u;
        }
    }
    if (sl == 0) piv[k] = p;
    if (best != 0.0) {
      if (p != k) {
        for (int j = sl; j < n; j += W) {
          const double a = A[j * n + k], b = A[j * n + p];
          A[j * n + k] = b;
          A[j * n + p] = a;
        }
      }
      lu_segment_fence();
      const double pivot = colk[k];
      for (int i = k + 1 + sl; i < n; i += W) colk[i] = colk[i] / pivot;
      lu_segment_fence();
    }
    double lik[kRows];                                // this lane's multipliers l(i, k)
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int i = k + 1 + sl + r * W;
      lik[r] = (i < n) ? colk[i] : 0.0;
    }
    const int rows = (n - (k + 1) - sl + W - 1) / W;  // rows of the trailing block this lane owns (<= 0: none)
    for (int j0 = k + 1; j0 < n; j0 += 4) {           // four columns of the rank-1 update at a time
      double ukj[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) ukj[c] = A[((j0 + c < n) ? j0 + c : n - 1) * n + k];
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        if (r < rows) {
          const int i = k + 1 + sl + r * W;
          double a[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) a[c] = A[((j0 + c < n) ? j0 + c : n - 1) * n + i];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (j0 + c < n) A[(j0 + c) * n + i] = a[c] - lik[r] * ukj[c];
        }
      }
    }
    lu_segment_fence();
  }
}

// value of `v` in lane `j` of the caller's segment
template <int W>
__device__ __forceinline__ double seg_lane_value(double v, int j) {
  return __shfl(v, j, W);
}

// lane i hands in b_i and gets x_i of LU x = P b back (n <= W; lanes >= n hand their value through untouched)
template <int W>
__device__ __forceinline__ double seg_lu_solve(const double* LU, const int* piv, double b, int n, int sl) {
  double x = b;
  for (int k = 0; k < n; ++k) {                       // the row interchanges, in order
    const int p = piv[k];
    const double xk = seg_lane_value<W>(x, k), xp = seg_lane_value<W>(x, p);
    x = (sl == k) ? xp : ((sl == p) ? xk : x);
  }
  for (int j = 0; j < n; ++j) {                       // unit lower triangle, column oriented
    const double xj = seg_lane_value<W>(x, j);
    if (sl > j && sl < n) x = x - xj * LU[j * n + sl];
  }
  for (int j = n - 1; j >= 0; --j) {                  // upper triangle, last column first
    const double xj = seg_lane_value<W>(x, j) / LU[j * n + j];
    if (sl == j) x = xj;
    if (sl < j) x = x - xj * LU[j * n + sl];
  }
  return x;
}

}  // namespace mi355
