// dispatch_trust_region.hip — the kernels of mi355_trust_region_newton_minimize_batch (trust_region_kernel.hpp): one
// coordinate per lane at 8, 16, 32 or 64 lanes per problem, on the built-in objectives whose functor has a hess_full
// (Rosenbrock, DiagQuadratic).  User functors with a hess_full get their own units (_build.py, trust_region=True).
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"
#include "trust_region_launch.hpp"

namespace mi355 {
namespace {
template <int W, int E>
struct RosenbrockOf {
  using type = RosenbrockConditionObjective;
};
template <int W, int E>
struct DiagQuadraticOf {
  using type = DiagQuadraticHessObjective<E>;
};
}  // namespace

int dispatch_trust_region(mi355_lbfgs_ctx* ctx, int W, int objective, const SolveArgs& args,
                          const TrustRegionDeviceConfig& cfg, hipStream_t stream) {
  return dispatch_builtin_or_user<kUserTrustRegion>(objective, &launch_trust_region_w<RosenbrockOf>, &launch_trust_region_w<DiagQuadraticOf>,
                                                    ctx, W, args, cfg, stream);
}

}  // namespace mi355
