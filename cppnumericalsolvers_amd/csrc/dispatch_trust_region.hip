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
  switch (objective) {
    case MI355_OBJ_ROSENBROCK:
      return launch_trust_region_w<RosenbrockOf>(ctx, W, args, cfg, stream);
    case MI355_OBJ_DIAG_QUADRATIC:
      return launch_trust_region_w<DiagQuadraticOf>(ctx, W, args, cfg, stream);
  }
  if (objective >= MI355_OBJ_USER_FIRST) {
    const UserTrustRegionFn fn = user_trust_region(objective);
    if (fn != nullptr) return fn(ctx, W, args, cfg, stream);
    return fail(MI355_ERR_UNSUPPORTED,
                "TrustRegionNewton: this library holds no trust-region kernel for this user objective (build it with "
                "trust_region=True and a functor that defines hess_full)");
  }
  return fail(MI355_ERR_UNSUPPORTED,
              "TrustRegionNewton is built for objectives with a device Hessian (hess_full): Rosenbrock, DiagQuadratic and "
              "user functors built with trust_region=True; the ridge forms and the augmented-Lagrangian composite have none");
}

}  // namespace mi355
