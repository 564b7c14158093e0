// trust_region_launch.hpp — launch of the trust-region kernel (trust_region_kernel.hpp) for one functor type, shared by
// dispatch_trust_region.hip (built-in objectives) and the units _build.py generates for user functors: the pre-checks and
// the LDS size here, the persistent-grid launch in solver_launch.hpp.
#pragma once
#include "trust_region_kernel.hpp"
#include "solver_launch.hpp"

namespace mi355 {

template <int W, class Obj>
int launch_trust_region(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const TrustRegionDeviceConfig& cfg, hipStream_t stream) {
  constexpr int kLdsLimit = 160 * 1024;
  if (args.n > W) return fail(MI355_ERR_INVALID_ARGUMENT, "TrustRegionNewton: lanes_per_problem must cover n");
  const int lds = (kWave / W) * trust_region_lds_doubles(args.n, W, args.hessian_condition_stop > 0.0) *
                  static_cast<int>(sizeof(double));
  if (lds > kLdsLimit) return fail(MI355_ERR_INVALID_ARGUMENT, "TrustRegionNewton: the Hessians do not fit LDS");
  return launch_persistent_solver<W, 1>(ctx, trust_region_kernel<W, Obj>, lds, args, cfg, stream);
}

// The four mappings: 8, 16, 32, 64 lanes at one coordinate per lane.  ObjOf<W, 1>::type is the functor type of a mapping.
template <template <int, int> class ObjOf>
int launch_trust_region_w(mi355_lbfgs_ctx* ctx, int W, const SolveArgs& args, const TrustRegionDeviceConfig& cfg,
                          hipStream_t stream) {
  switch (W) {
    case 8: return launch_trust_region<8, typename ObjOf<8, 1>::type>(ctx, args, cfg, stream);
    case 16: return launch_trust_region<16, typename ObjOf<16, 1>::type>(ctx, args, cfg, stream);
    case 32: return launch_trust_region<32, typename ObjOf<32, 1>::type>(ctx, args, cfg, stream);
    case 64: return launch_trust_region<64, typename ObjOf<64, 1>::type>(ctx, args, cfg, stream);
  }
  return fail(MI355_ERR_INVALID_ARGUMENT, "TrustRegionNewton: lanes_per_problem must be 8, 16, 32 or 64");
}

}  // namespace mi355
