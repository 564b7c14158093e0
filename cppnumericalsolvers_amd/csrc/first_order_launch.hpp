// first_order_launch.hpp — launch of the first-order kernel (first_order_kernel.hpp) for one functor type, shared by
// dispatch_first_order.hip (built-in objectives) and the units _build.py generates for user functors: the pre-check here,
// the persistent-grid launch in solver_launch.hpp (no dynamic LDS).
#pragma once
#include "first_order_kernel.hpp"
#include "solver_launch.hpp"

namespace mi355 {

template <int W, int E, int Method, class Obj>
int launch_first_order(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const FirstOrderDeviceConfig& cfg, hipStream_t stream) {
  if (args.n > W * E) return fail(MI355_ERR_INVALID_ARGUMENT, "first-order solver: the lane mapping must cover n");
  return launch_persistent_solver<W, E>(ctx, first_order_kernel<W, E, Method, Obj>, 0, args, cfg, stream);
}

// The six built mappings: 8, 16, 32, 64 lanes at one coordinate per lane, 64 lanes at two and four.  ObjOf<W, E>::type
// is the functor type of a mapping (DiagQuadraticObjective is a template over E).
template <int Method, template <int, int> class ObjOf>
int launch_first_order_we(mi355_lbfgs_ctx* ctx, int W, int E, const SolveArgs& args, const FirstOrderDeviceConfig& cfg,
                          hipStream_t stream) {
  if (E == 1) {
    switch (W) {
      case 8: return launch_first_order<8, 1, Method, typename ObjOf<8, 1>::type>(ctx, args, cfg, stream);
      case 16: return launch_first_order<16, 1, Method, typename ObjOf<16, 1>::type>(ctx, args, cfg, stream);
      case 32: return launch_first_order<32, 1, Method, typename ObjOf<32, 1>::type>(ctx, args, cfg, stream);
      case 64: return launch_first_order<64, 1, Method, typename ObjOf<64, 1>::type>(ctx, args, cfg, stream);
    }
  } else if (W == 64 && E == 2) {
    return launch_first_order<64, 2, Method, typename ObjOf<64, 2>::type>(ctx, args, cfg, stream);
  } else if (W == 64 && E == 4) {
    return launch_first_order<64, 4, Method, typename ObjOf<64, 4>::type>(ctx, args, cfg, stream);
  }
  return fail(MI355_ERR_INVALID_ARGUMENT,
              "first-order solver: the mapping must be 8, 16, 32 or 64 lanes at one coordinate per lane, or 64 lanes at "
              "two or four");
}

template <template <int, int> class ObjOf>
int launch_first_order_method(mi355_lbfgs_ctx* ctx, int method, int W, int E, const SolveArgs& args,
                              const FirstOrderDeviceConfig& cfg, hipStream_t stream) {
  if (method == kGradientDescent)
    return launch_first_order_we<kGradientDescent, ObjOf>(ctx, W, E, args, cfg, stream);
  return launch_first_order_we<kConjugatedGradientDescent, ObjOf>(ctx, W, E, args, cfg, stream);
}

}  // namespace mi355
