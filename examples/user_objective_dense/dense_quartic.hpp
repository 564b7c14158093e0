// dense_quartic.hpp — a USER functor with a DENSE device Hessian, for TrustRegionNewton and NewtonDescent (worked example
// and the test functor of the dense linear algebra: csrc/lu_device.hpp, hessian_condition_device.hpp, the column walk of
// newton_descent_kernel.hpp and the row walk of trust_region_kernel.hpp).
//
//     f(x) = 0.5 x . (S x) - b . x + (kappa / 4) sum_i x_i^4,   g = S x - b + kappa x^3,   H = S + 3 kappa diag(x^2)
//
// S (n x n, COLUMN MAJOR: S(i, j) at S[j n + i]), b (n) and kappa are shared by the batch: objective_params holds
// n n + n + 1 doubles in that order.  S is used as given: the functor never symmetrises, H(i, j) = S(i, j) is stored at
// Hm[j n + i], so a solver that reads H(j, i) for H(i, j) computes something else whenever S != S^T.
//     _build.build(output=".../libmi355_lbfgs_tr.so",
//                  user_objectives=[..., dict(name="dense_quartic", header=<this file>, type="user_examples::DenseQuartic",
//                                             id=101, lbfgs=True, lbfgsb=False, trust_region=True, newton_descent=True)])
// lbfgs=True also builds the Lbfgs kernels: with hessian_from_functor they take the preconditioner from hess_diag and,
// with the condition_hessian test on, H(x) from hess_full at one or two coordinates per lane — the only place where the
// condition number's LU meets a dense matrix with two rows of the trailing block per lane.
// Operation order (tests/newton_descent/nd_twin.hpp, tests/trust_region/tr_twin.hpp and the two reference harnesses state
// the same), per coordinate i:
//     sx_i = S(i, 0) x_0, then sx_i = sx_i + S(i, j) x_j for j = 1 .. n - 1           (ascending, first term a product)
//     q_i = x_i x_i,   g_i = (sx_i - b_i) + kappa (q_i x_i),   H(i, i) = S(i, i) + (3 kappa) q_i
//     f = (0.5 sum_i x_i sx_i - sum_i b_i x_i) + (0.25 kappa) sum_i q_i q_i          (the three sums: the segment sum)
// x_j of another lane comes out of seg_coordinate: a butterfly over x_j and zeros, exact (a -0.0 arrives as +0.0).
#pragma once

namespace user_examples {

struct DenseQuartic {
  static constexpr int kLdsDoubles = 0;
  __host__ __device__ static constexpr int shared_lds_doubles() { return 0; }
  const double* S;
  const double* b;
  double kappa;
  __device__ __forceinline__ void load(const double* params, int n, int, double*, double*) {
    S = params;
    b = params + n * n;
    kappa = params[n * n + n];
  }
  __device__ __forceinline__ void begin_problem(const double*, long long, int, int) {}

  // row sl * E + e of S x; every lane of the segment takes part in every seg_coordinate, padding lanes keep 0
  template <int W, int E>
  __device__ __forceinline__ void times_s(const double (&x)[E], double (&sx)[E], int n, int sl) const {
#pragma unroll
    for (int e = 0; e < E; ++e) sx[e] = 0.0;
    for (int j = 0; j < n; ++j) {
      const double xj = mi355::seg_coordinate<W, E>(x, j, sl);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = sl * E + e;
        if (i < n) sx[e] = (j == 0) ? S[i] * xj : sx[e] + S[j * n + i] * xj;
      }
    }
  }
  template <int W, int E>
  __device__ __forceinline__ double finish(const double (&x)[E], const double (&sx)[E], int n, int sl) const {
    double quad = 0.0, lin = 0.0, quart = 0.0;   // E > 1: ascending over the lane's coordinates, then the segment sum
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = sl * E + e;
      const double q = x[e] * x[e];
      const double t0 = (i < n) ? x[e] * sx[e] : 0.0;
      const double t1 = (i < n) ? b[i] * x[e] : 0.0;
      const double t2 = (i < n) ? q * q : 0.0;
      quad = (e == 0) ? t0 : quad + t0;
      lin = (e == 0) ? t1 : lin + t1;
      quart = (e == 0) ? t2 : quart + t2;
    }
    const double sq = mi355::seg_sum<W>(quad);
    const double sb = mi355::seg_sum<W>(lin);
    const double s4 = mi355::seg_sum<W>(quart);
    return (0.5 * sq - sb) + (0.25 * kappa) * s4;
  }

  template <int W, int E>
  __device__ __forceinline__ double eval(const double (&x)[E], double (&g)[E], int n, int sl) const {
    double sx[E];
    times_s<W, E>(x, sx, n, sl);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = sl * E + e;
      const double q = x[e] * x[e];
      g[e] = (i < n) ? (sx[e] - b[i]) + kappa * (q * x[e]) : 0.0;
    }
    return finish<W, E>(x, sx, n, sl);
  }
  // the value alone: the same products and sums
  template <int W, int E>
  __device__ __forceinline__ double value(const double (&x)[E], int n, int sl) const {
    double sx[E];
    times_s<W, E>(x, sx, n, sl);
    return finish<W, E>(x, sx, n, sl);
  }
  // diag H(x) for Lbfgs in Second mode (hessian_from_functor: the preconditioner of every iterate): the diagonal of
  // hess_full, the same operations; padding coordinates 0
  template <int W, int E>
  __device__ __forceinline__ void hess_diag(const double (&x)[E], double (&h)[E], int n, int sl) const {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = sl * E + e;
      h[e] = (i < n) ? S[i * n + i] + (3.0 * kappa) * (x[e] * x[e]) : 0.0;
    }
  }
  template <int W, int E>
  __device__ __forceinline__ void hess_full(const double (&x)[E], double* Hm, int n, int sl) const {
    for (int t = sl; t < n * n; t += W) Hm[t] = S[t];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = sl * E + e;
      if (i < n) Hm[i * n + i] = S[i * n + i] + (3.0 * kappa) * (x[e] * x[e]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

}  // namespace user_examples
