// dispatch_newton_descent.hip — the kernels of mi355_newton_descent_minimize_batch (newton_descent_kernel.hpp): one
// coordinate per lane at 8, 16, 32 or 64 lanes per problem, on the built-in objectives whose functor has a hess_full
// (Rosenbrock, DiagQuadratic).  User functors with a hess_full get their own units (_build.py, newton_descent=True).
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"
#include "newton_descent_launch.hpp"

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

int dispatch_newton_descent(mi355_lbfgs_ctx* ctx, int W, int objective, const SolveArgs& args,
                            const NewtonDescentDeviceConfig& cfg, hipStream_t stream) {
  return dispatch_builtin_or_user<kUserNewtonDescent>(objective, &launch_newton_descent_w<RosenbrockOf>, &launch_newton_descent_w<DiagQuadraticOf>,
                                                      ctx, W, args, cfg, stream);
}

}  // namespace mi355
