// nelder_mead_launch.hpp — launch of the Nelder-Mead kernel (nelder_mead_kernel.hpp) for one functor type, shared by
// dispatch_nelder_mead.hip (built-in objectives) and the units _build.py generates for user functors: the mode, the
// LDS size and its limit here, the persistent-grid launch in solver_launch.hpp.
#pragma once
#include "nelder_mead_kernel.hpp"
#include "solver_launch.hpp"

namespace mi355 {

template <int W, class Obj, bool FIRST>
int launch_nelder_mead_mode(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const NelderMeadDeviceConfig& cfg,
                            hipStream_t stream) {
  constexpr int kLdsLimit = 160 * 1024;
  const int lds = (kWave / W) * nelder_mead_lds_doubles(args.n, W) * static_cast<int>(sizeof(double));
  if (lds > kLdsLimit) return fail(MI355_ERR_INVALID_ARGUMENT, "NelderMead: the simplices do not fit LDS");
  return launch_persistent_solver<W, 1>(ctx, nelder_mead_kernel<W, Obj, FIRST>, lds, args, cfg, stream);
}

// value mode for every functor; first mode for those with a value-and-gradient entry (eval)
template <int W, class Obj>
int launch_nelder_mead(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const NelderMeadDeviceConfig& cfg, hipStream_t stream) {
  if (!cfg.first_mode) return launch_nelder_mead_mode<W, Obj, false>(ctx, args, cfg, stream);
  if constexpr (HasGradientEval<Obj>::value) {
    return launch_nelder_mead_mode<W, Obj, true>(ctx, args, cfg, stream);
  } else {
    return fail(MI355_ERR_INVALID_ARGUMENT, "NelderMead: this functor is value-only (no eval): value mode only");
  }
}

// The four mappings: 8, 16, 32, 64 lanes at one coordinate per lane.  ObjOf<W, 1>::type is the functor type of a mapping.
template <template <int, int> class ObjOf>
int launch_nelder_mead_w(mi355_lbfgs_ctx* ctx, int W, const SolveArgs& args, const NelderMeadDeviceConfig& cfg,
                         hipStream_t stream) {
  return launch_for_lanes(W, [&](auto w) {
    return launch_nelder_mead<decltype(w)::value, typename ObjOf<decltype(w)::value, 1>::type>(ctx, args, cfg, stream);
  });
}

}  // namespace mi355
