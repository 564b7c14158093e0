// quartic.hpp — a USER functor with a device Hessian, for TrustRegionNewton, NewtonDescent and the first-order solvers
// (GradientDescent, ConjugatedGradientDescent) (worked example).
//
// The reference's trust_region_newton_test.cc minimises the 1-D double well f(x) = (x^2 - 2)^2 from a start next to its
// local maximum at 0.  On the device the function is a functor with the interface of
// cppnumericalsolvers_amd/csrc/objectives.hpp plus hess_full (H n x n, column major, in the segment's LDS); a build of the
// library compiles it into the trust-region, Newton-descent and first-order kernels only:
//     _build.build(output=".../libmi355_lbfgs_tr.so",
//                  user_objectives=[dict(name="quartic", header=<this file>, type="user_examples::QuarticDoubleWell",
//                                        id=100, lbfgs=False, lbfgsb=False, trust_region=True, newton_descent=True,
//                                        first_order=True)])
// In more than one dimension the function still reads x_0 alone (g and H are zero elsewhere).
// Operation order: t = x x - 2, f = t t, g = (4 x) t, H = (12 x) x - 8 (tests/trust_region/tr_twin.hpp states the same).
#pragma once

namespace user_examples {

struct QuarticDoubleWell {
  static constexpr int kLdsDoubles = 0;
  __host__ __device__ static constexpr int shared_lds_doubles() { return 0; }
  __device__ __forceinline__ void load(const double*, int, int, double*, double*) {}
  __device__ __forceinline__ void begin_problem(const double*, long long, int, int) {}

  template <int W, int E>
  __device__ __forceinline__ double eval(const double (&x)[E], double (&g)[E], int, int sl) const {
    const double x0 = mi355::seg_coordinate<W, E>(x, 0, sl);
    const double t = x0 * x0 - 2.0;
#pragma unroll
    for (int e = 0; e < E; ++e) g[e] = (sl * E + e == 0) ? (4.0 * x0) * t : 0.0;
    return t * t;
  }
  // the value alone (the Armijo trials of ConjugatedGradientDescent): the same t, the same product
  template <int W, int E>
  __device__ __forceinline__ double value(const double (&x)[E], int, int sl) const {
    const double x0 = mi355::seg_coordinate<W, E>(x, 0, sl);
    const double t = x0 * x0 - 2.0;
    return t * t;
  }
  template <int W, int E>
  __device__ __forceinline__ void hess_full(const double (&x)[E], double* Hm, int n, int sl) const {
    const double x0 = mi355::seg_coordinate<W, E>(x, 0, sl);
    // (n > 1: the function reads x_0 alone, every other entry of H is zero)
    for (int t = sl; t < n * n; t += W) Hm[t] = (t == 0) ? (12.0 * x0) * x0 - 8.0 : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

}  // namespace user_examples
