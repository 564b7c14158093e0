// dispatch_lbfgsb_fast_own_box.hip — the relaxed-algebra L-BFGS-B kernels with one box per problem (lbfgsb_fast_kernel<...,
// OwnBox = true>; see engine_internal.hpp): Rosenbrock / DiagQuadratic, one or two coordinates per lane (n <= 32, the
// unstaged form with the box in registers), capacity 5 and 8.
#include "lbfgsb_fast_dispatch.hpp"

namespace mi355 {
namespace {
template <int E, class Obj>
int by_capacity(mi355_lbfgs_ctx* ctx, const LbfgsbArgs& args, hipStream_t stream) {
  if (args.s.m <= 5) return launch_lbfgsb_fast<E, Obj, 5, true>(ctx, args, stream);
  if (args.s.m <= 8) return launch_lbfgsb_fast<E, Obj, 8, true>(ctx, args, stream);
  return fail(MI355_ERR_UNSUPPORTED, "relaxed-algebra L-BFGS-B with per-problem bounds is built for m <= 8");
}
template <int E>
int by_objective(mi355_lbfgs_ctx* ctx, int objective, const LbfgsbArgs& args, hipStream_t stream) {
  switch (objective) {
    case MI355_OBJ_ROSENBROCK: return by_capacity<E, RosenbrockObjective>(ctx, args, stream);
    case MI355_OBJ_DIAG_QUADRATIC: return by_capacity<E, DiagQuadraticObjective<E>>(ctx, args, stream);
  }
  return fail(MI355_ERR_UNSUPPORTED, "relaxed-algebra L-BFGS-B with per-problem bounds: Rosenbrock and DiagQuadratic only");
}
}  // namespace

int dispatch_lbfgsb_fast_own_box(mi355_lbfgs_ctx* ctx, int E, int objective, const LbfgsbArgs& args, hipStream_t stream) {
  switch (E) {
    case 1: return by_objective<1>(ctx, objective, args, stream);
    case 2: return by_objective<2>(ctx, objective, args, stream);
  }
  return fail(MI355_ERR_UNSUPPORTED, "relaxed-algebra L-BFGS-B with per-problem bounds is built for n <= 32");
}
}  // namespace mi355
