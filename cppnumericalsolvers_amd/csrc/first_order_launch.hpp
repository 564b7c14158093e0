// first_order_launch.hpp — launch of the first-order kernel (first_order_kernel.hpp) for one functor type, shared by
// dispatch_first_order.hip (built-in objectives) and the units _build.py generates for user functors: the six
// lane mappings and the two methods here, the persistent-grid launch in solver_launch.hpp (no dynamic LDS).
#pragma once
#include "first_order_kernel.hpp"
#include "solver_launch.hpp"

namespace mi355 {

template <int W, int E, int Method, class Obj>
int launch_first_order(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const FirstOrderDeviceConfig& cfg, hipStream_t stream) {
  return launch_persistent_solver<W, E>(ctx, first_order_kernel<W, E, Method, Obj>, 0, args, cfg, stream);
}

// The six built mappings: 8, 16, 32, 64 lanes at one coordinate per lane, 64 lanes at two and four.  ObjOf<W, E>::type
// is the functor type of a mapping (DiagQuadraticObjective is a template over E).
template <int Method, template <int, int> class ObjOf>
int launch_first_order_we(mi355_lbfgs_ctx* ctx, int W, int E, const SolveArgs& args, const FirstOrderDeviceConfig& cfg,
                          hipStream_t stream) {
  if (E == 1)
    return launch_for_lanes(W, [&](auto w) {
      return launch_first_order<decltype(w)::value, 1, Method, typename ObjOf<decltype(w)::value, 1>::type>(ctx, args, cfg, stream);
    });
  if (W == 64 && E == 2) return launch_first_order<64, 2, Method, typename ObjOf<64, 2>::type>(ctx, args, cfg, stream);
  if (W == 64 && E == 4) return launch_first_order<64, 4, Method, typename ObjOf<64, 4>::type>(ctx, args, cfg, stream);
  return fail(MI355_ERR_INVALID_ARGUMENT, "internal: no first-order kernel for this (W, E)");
}

template <template <int, int> class ObjOf>
int launch_first_order_method(mi355_lbfgs_ctx* ctx, int method, int W, int E, const SolveArgs& args,
                              const FirstOrderDeviceConfig& cfg, hipStream_t stream) {
  if (method == kGradientDescent)
    return launch_first_order_we<kGradientDescent, ObjOf>(ctx, W, E, args, cfg, stream);
  return launch_first_order_we<kConjugatedGradientDescent, ObjOf>(ctx, W, E, args, cfg, stream);
}

}  // namespace mi355
