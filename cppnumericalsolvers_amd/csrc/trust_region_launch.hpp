// trust_region_launch.hpp — launch of the trust-region kernel (trust_region_kernel.hpp) for one functor type, shared by
// dispatch_trust_region.hip (built-in objectives) and the units _build.py generates for user functors: the LDS size
// and its limit here, the persistent-grid launch in solver_launch.hpp.
#pragma once
#include "trust_region_kernel.hpp"
#include "solver_launch.hpp"

namespace mi355 {

template <int W, class Obj>
int launch_trust_region(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const TrustRegionDeviceConfig& cfg, hipStream_t stream) {
  constexpr int kLdsLimit = 160 * 1024;
  const int lds = (kWave / W) * trust_region_lds_doubles(args.n, W, args.hessian_condition_stop > 0.0) *
                  static_cast<int>(sizeof(double));
  if (lds > kLdsLimit) return fail(MI355_ERR_INVALID_ARGUMENT, "TrustRegionNewton: the Hessians do not fit LDS");
  return launch_persistent_solver<W, 1>(ctx, trust_region_kernel<W, Obj>, lds, args, cfg, stream);
}

// The four mappings: 8, 16, 32, 64 lanes at one coordinate per lane.  ObjOf<W, 1>::type is the functor type of a mapping.
template <template <int, int> class ObjOf>
int launch_trust_region_w(mi355_lbfgs_ctx* ctx, int W, const SolveArgs& args, const TrustRegionDeviceConfig& cfg,
                          hipStream_t stream) {
  return launch_for_lanes(W, [&](auto w) {
    return launch_trust_region<decltype(w)::value, typename ObjOf<decltype(w)::value, 1>::type>(ctx, args, cfg, stream);
  });
}

}  // namespace mi355
