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
  return dispatch_builtin_or_user<kUserFirstOrder>(objective, &launch_first_order_method<RosenbrockOf>, &launch_first_order_method<DiagQuadraticOf>,
                                                   ctx, method, W, E, args, cfg, stream);
}

}  // namespace mi355
