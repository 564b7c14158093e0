// The lean solve kernels: the flagship shapes with the launch options fixed at compile time (LeanOptions, lbfgs_kernel.hpp).
// Four kernels — Rosenbrock filling its segment, fused arithmetic, More-Thuente, 8 x 4 and 16 x 4 lanes x coordinates,
// six and ten y columns in registers — in a unit of their own, so that no other unit grows and the cold build stays
// parallel.  launch_solve_rosenbrock_full (engine_internal.hpp) decides when they run; every other call takes the general
// kernel of dispatch_w8.hip / dispatch_w16.hip.
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"

namespace mi355 {

namespace {
template <int W>
int launch_lean(mi355_lbfgs_ctx* ctx, int mr, const SolveArgs& args, hipStream_t stream) {
  using Obj = RosenbrockFullObjective;
  constexpr int MT = MI355_LS_MORE_THUENTE;
  return mr == 6 ? launch_solve<W, 4, Obj, 6, MT, kAlgLbfgs, NoOuterLoop, ArithFma, LeanOptions>(ctx, args, stream)
                 : launch_solve<W, 4, Obj, 10, MT, kAlgLbfgs, NoOuterLoop, ArithFma, LeanOptions>(ctx, args, stream);
}
}  // namespace

int dispatch_lean(mi355_lbfgs_ctx* ctx, int W, int mr, const SolveArgs& args, hipStream_t stream) {
  if (mr < 6 || mr > 10 || args.n != W * 4)
    return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the lean solve kernels hold m = 6..10 at n = 4 x lanes_per_problem");
  switch (W) {
    case 8: return launch_lean<8>(ctx, mr, args, stream);
    case 16: return launch_lean<16>(ctx, mr, args, stream);
  }
  return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the lean solve kernels are built for 8 and 16 lanes per problem");
}

}  // namespace mi355
