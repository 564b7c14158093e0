// dispatch_lbfgsb_own_box.hip — the reference-order L-BFGS-B kernels with one box per problem (lbfgsb_solve_kernel<...,
// OwnBox = true>; see engine_internal.hpp).  A bounded set, in a unit of its own: More-Thuente, sixteen lanes per problem,
// one, two or four coordinates per lane (n <= 64); capacity 5 and 8 on Rosenbrock / DiagQuadratic, capacity 5 on the ridge
// objective.
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"

namespace mi355 {
namespace {
constexpr int MT = MI355_LS_MORE_THUENTE;
template <int E, class Obj>
int by_capacity(mi355_lbfgs_ctx* ctx, const LbfgsbArgs& args, hipStream_t stream) {
  if (args.s.m <= 5) return launch_lbfgsb<E, Obj, 5, MT, NoOuterLoop, 16, true>(ctx, args, stream);
  if constexpr (Obj::shared_lds_doubles() == 0) {
    if (args.s.m <= 8) return launch_lbfgsb<E, Obj, 8, MT, NoOuterLoop, 16, true>(ctx, args, stream);
  }
  return fail(MI355_ERR_UNSUPPORTED, "L-BFGS-B with per-problem bounds: no kernel of this history size on this objective");
}
template <int E>
int by_objective(mi355_lbfgs_ctx* ctx, int objective, const LbfgsbArgs& args, hipStream_t stream) {
  switch (objective) {
    case MI355_OBJ_ROSENBROCK: return by_capacity<E, RosenbrockObjective>(ctx, args, stream);
    case MI355_OBJ_DIAG_QUADRATIC: return by_capacity<E, DiagQuadraticObjective<E>>(ctx, args, stream);
    case MI355_OBJ_SQUARED_ERROR_RIDGE: return by_capacity<E, SquaredErrorRidgeObjective<16, E>>(ctx, args, stream);
  }
  return fail(MI355_ERR_UNSUPPORTED, "L-BFGS-B with per-problem bounds: no kernel for this objective");
}
}  // namespace

int dispatch_lbfgsb_own_box(mi355_lbfgs_ctx* ctx, int E, int objective, const LbfgsbArgs& args, hipStream_t stream) {
  switch (E) {
    case 1: return by_objective<1>(ctx, objective, args, stream);
    case 2: return by_objective<2>(ctx, objective, args, stream);
    case 4: return by_objective<4>(ctx, objective, args, stream);
  }
  return fail(MI355_ERR_UNSUPPORTED, "L-BFGS-B with per-problem bounds is built for n <= 64");
}
}  // namespace mi355
