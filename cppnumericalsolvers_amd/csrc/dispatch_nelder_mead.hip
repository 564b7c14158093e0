// dispatch_nelder_mead.hip — the kernels of mi355_nelder_mead_minimize_batch (nelder_mead_kernel.hpp): one coordinate
// per lane at 8, 16, 32 or 64 lanes per problem, value mode and first mode, on Rosenbrock and DiagQuadratic.  User
// functors get their own units (_build.py, nelder_mead=True).
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"
#include "nelder_mead_launch.hpp"

namespace mi355 {
namespace {
template <int W, int E>
struct RosenbrockOf {
  using type = RosenbrockObjective;
};
template <int W, int E>
struct DiagQuadraticOf {
  using type = DiagQuadraticObjective<E>;
};
}  // namespace

int dispatch_nelder_mead(mi355_lbfgs_ctx* ctx, int W, int objective, const SolveArgs& args,
                         const NelderMeadDeviceConfig& cfg, hipStream_t stream) {
  return dispatch_builtin_or_user<kUserNelderMead>(objective, &launch_nelder_mead_w<RosenbrockOf>, &launch_nelder_mead_w<DiagQuadraticOf>,
                                                   ctx, W, args, cfg, stream);
}

}  // namespace mi355
