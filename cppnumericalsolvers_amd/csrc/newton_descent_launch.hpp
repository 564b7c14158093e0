// newton_descent_launch.hpp — launch of the Newton-descent kernel (newton_descent_kernel.hpp) for one functor type, shared by
// dispatch_newton_descent.hip (built-in objectives) and the units _build.py generates for user functors: the LDS size
// and its limit here, the persistent-grid launch in solver_launch.hpp.
#pragma once
#include "newton_descent_kernel.hpp"
#include "solver_launch.hpp"

namespace mi355 {

template <int W, class Obj>
int launch_newton_descent(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const NewtonDescentDeviceConfig& cfg, hipStream_t stream) {
  constexpr int kLdsLimit = 160 * 1024;
  const int lds = (kWave / W) * newton_descent_lds_doubles(args.n, W, args.hessian_condition_stop > 0.0) *
                  static_cast<int>(sizeof(double));
  if (lds > kLdsLimit) return fail(MI355_ERR_INVALID_ARGUMENT, "NewtonDescent: the Hessians and their LU copies do not fit LDS");
  return launch_persistent_solver<W, 1>(ctx, newton_descent_kernel<W, Obj>, lds, args, cfg, stream);
}

// The four mappings: 8, 16, 32, 64 lanes at one coordinate per lane.  ObjOf<W, 1>::type is the functor type of a mapping.
template <template <int, int> class ObjOf>
int launch_newton_descent_w(mi355_lbfgs_ctx* ctx, int W, const SolveArgs& args, const NewtonDescentDeviceConfig& cfg,
                            hipStream_t stream) {
  return launch_for_lanes(W, [&](auto w) {
    return launch_newton_descent<decltype(w)::value, typename ObjOf<decltype(w)::value, 1>::type>(ctx, args, cfg, stream);
  });
}

}  // namespace mi355
