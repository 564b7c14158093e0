// l1_quadratic.hpp — a VALUE-ONLY user functor, for NelderMead (worked example).
//
//     f(x) = sum_i |x_i - c_i| + 0.5 sum_i (x_i - c_i)^2
// is non-smooth exactly at its minimiser x = c: it has a value and nothing else, the case only the derivative-free solver
// takes.  On the device the function is a functor with load / begin_problem of cppnumericalsolvers_amd/csrc/objectives.hpp
// and a value<W, E> entry instead of eval; a build of the library compiles it into the Nelder-Mead kernels only:
//     _build.build(output=".../libmi355_lbfgs_nm.so",
//                  user_objectives=[dict(name="l1_quadratic", header=<this file>, type="user_examples::L1Quadratic",
//                                        id=100, lbfgs=False, lbfgsb=False, nelder_mead=True)])
// Parameters: c[0..n).  Operation order: d = x_i - c_i, term_i = |d| + (0.5 d) d, f = the segment sum of the terms.
#pragma once

namespace user_examples {

struct L1Quadratic {
  static constexpr int kLdsDoubles = 0;
  __host__ __device__ static constexpr int shared_lds_doubles() { return 0; }
  double c_reg;
  __device__ __forceinline__ void load(const double* params, int n, int sl, double*, double*) {
    c_reg = (sl < n) ? params[sl] : 0.0;
  }
  __device__ __forceinline__ void begin_problem(const double*, long long, int, int) {}

  template <int W, int E>
  __device__ __forceinline__ double value(const double (&x)[E], int n, int sl) const {
    static_assert(E == 1, "one coordinate per lane");
    const double d = x[0] - c_reg;
    const double term = (sl < n) ? __builtin_fabs(d) + (0.5 * d) * d : 0.0;
    return mi355::seg_sum<W>(term);
  }
};

}  // namespace user_examples
