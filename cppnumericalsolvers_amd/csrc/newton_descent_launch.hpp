// newton_descent_launch.hpp — launch of the Newton-descent kernel (newton_descent_kernel.hpp) for one functor type, shared by
// dispatch_newton_descent.hip (built-in objectives) and the units _build.py generates for user functors: the pre-checks and
// the LDS size here, the persistent-grid launch in solver_launch.hpp.
#pragma once
#include "newton_descent_kernel.hpp"
#include "solver_launch.hpp"

namespace mi355 {

template <int W, class Obj>
int launch_newton_descent(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const NewtonDescentDeviceConfig& cfg, hipStream_t stream) {
  constexpr int kLdsLimit = 160 * 1024;
  if (args.n > W) return fail(MI355_ERR_INVALID_ARGUMENT, "NewtonDescent: lanes_per_problem must cover n");
  const int lds = (kWave / W) * newton_descent_lds_doubles(args.n, W, args.hessian_condition_stop > 0.0) *
                  static_cast<int>(sizeof(double));
  if (lds > kLdsLimit) return fail(MI355_ERR_INVALID_ARGUMENT, "NewtonDescent: the Hessians and their LU copies do not fit LDS");
  return launch_persistent_solver<W, 1>(ctx, newton_descent_kernel<W, Obj>, lds, args, cfg, stream);
}

// The four mappings: 8, 16, 32, 64 lanes at one coordinate per lane.  ObjOf<W, 1>::type is the functor type of a mapping.
template <template <int, int> class ObjOf>
int launch_newton_descent_w(mi355_lbfgs_ctx* ctx, int W, const SolveArgs& args, const NewtonDescentDeviceConfig& cfg,
                            hipStream_t stream) {
  switch (W) {
    case 8: return launch_newton_descent<8, typename ObjOf<8, 1>::type>(ctx, args, cfg, stream);
    case 16: return launch_newton_descent<16, typename ObjOf<16, 1>::type>(ctx, args, cfg, stream);
    case 32: return launch_newton_descent<32, typename ObjOf<32, 1>::type>(ctx, args, cfg, stream);
    case 64: return launch_newton_descent<64, typename ObjOf<64, 1>::type>(ctx, args, cfg, stream);
  }
  return fail(MI355_ERR_INVALID_ARGUMENT, "NewtonDescent: lanes_per_problem must be 8, 16, 32 or 64");
}

}  // namespace mi355
