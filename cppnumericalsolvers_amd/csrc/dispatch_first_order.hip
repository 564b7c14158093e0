// dispatch_first_order.hip — the kernels of mi355_gradient_descent_minimize_batch and
// mi355_conjugated_gradient_descent_minimize_batch (first_order_kernel.hpp): six lane mappings per method on the
// built-in objectives without LDS data (Rosenbrock, DiagQuadratic).  User functors get their own units (_build.py,
// first_order=True).
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"
#include "first_order_launch.hpp"

namespace mi355 {
namespace {
template <int W, int E>
struct RosenbrockOf {
  using type = RosenbrockObjectiveT<false>;
};
template <int W, int E>
struct DiagQuadraticOf {
  using type = DiagQuadraticObjective<E>;
};
}  // namespace

int dispatch_first_order(mi355_lbfgs_ctx* ctx, int method, int W, int E, int objective, const SolveArgs& args,
                         const FirstOrderDeviceConfig& cfg, hipStream_t stream) {
  switch (objective) {
    case MI355_OBJ_ROSENBROCK:
      return launch_first_order_method<RosenbrockOf>(ctx, method, W, E, args, cfg, stream);
    case MI355_OBJ_DIAG_QUADRATIC:
      return launch_first_order_method<DiagQuadraticOf>(ctx, method, W, E, args, cfg, stream);
  }
  if (objective >= MI355_OBJ_USER_FIRST) {
    const UserFirstOrderFn fn = user_first_order(objective);
    if (fn != nullptr) return fn(ctx, method, W, E, args, cfg, stream);
    return fail(MI355_ERR_UNSUPPORTED,
                "GradientDescent / ConjugatedGradientDescent: this library holds no first-order kernel for this user "
                "objective (build it with first_order=True)");
  }
  return fail(MI355_ERR_UNSUPPORTED,
              "GradientDescent / ConjugatedGradientDescent are built for objectives without LDS data: Rosenbrock, "
              "DiagQuadratic and user functors built with first_order=True; not the ridge forms or the "
              "augmented-Lagrangian composite");
}

}  // namespace mi355
