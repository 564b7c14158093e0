// solver_launch.hpp — what the dispatch units of TrustRegionNewton, NewtonDescent, NelderMead and the first-order solvers
// share on the host: the built-in / user fork, the choice among the four lane counts, and the persistent-grid launch
// (everything from the occupancy query to the context's record of the launch).  The four launch headers keep their own
// LDS formula.  Unlike launch_solve (engine_internal.hpp) the launch always records ev_start (no caller of these solvers
// arms it) and always hands the kernel the plateau-ring scratch.  The entry points (solver_entry.hip) refuse what has no
// kernel, with the reason; what they let through by mistake meets one of the "internal:" lines here.
#pragma once
#include <type_traits>

#include "engine_internal.hpp"

namespace mi355 {

// The fork every dispatch unit takes: its own launch function on the functor family of a built-in objective, or the
// function the generated unit of a user objective registered in slot S; `a`: everything but the objective id.
template <UserSolver S, class... A>
int dispatch_builtin_or_user(int objective, typename UserSolverSignature<S>::Fn rosenbrock,
                             typename UserSolverSignature<S>::Fn diag_quadratic, const A&... a) {
  const auto fn = objective == MI355_OBJ_ROSENBROCK       ? rosenbrock
                  : objective == MI355_OBJ_DIAG_QUADRATIC ? diag_quadratic
                                                          : user_solver_fn<S>(objective);
  return fn ? fn(a...) : fail(MI355_ERR_UNSUPPORTED, "internal: this solver holds no kernel for the objective");
}

// launch(std::integral_constant<int, W>()) for the W of the call: 8, 16, 32 or 64 lanes per problem
template <class Launch>
int launch_for_lanes(int W, Launch launch) {
  switch (W) {
    case 8: return launch(std::integral_constant<int, 8>());
    case 16: return launch(std::integral_constant<int, 16>());
    case 32: return launch(std::integral_constant<int, 32>());
    case 64: return launch(std::integral_constant<int, 64>());
  }
  return fail(MI355_ERR_INVALID_ARGUMENT, "internal: lanes_per_problem is not 8, 16, 32 or 64");
}

// kern: a __global__ function taking (SolveArgs, Config), one wavefront per workgroup, W lanes per problem at E
// coordinates per lane; lds: its dynamic LDS bytes (0: none, and the kernel's limit is left alone)
template <int W, int E, class Kernel, class Config>
int launch_persistent_solver(mi355_lbfgs_ctx* ctx, Kernel kern, int lds, SolveArgs args, const Config& cfg,
                             hipStream_t stream) {
  constexpr int kSegs = kWave / W;
  if (args.n > W * E) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the lane mapping does not cover n");
  if (lds > 0)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWave, lds));
  if (per_cu < 1) per_cu = 1;
  const long long blocks_needed = (args.B + kSegs - 1) / kSegs;
  long long blocks_ll = static_cast<long long>(per_cu) * ctx->num_cus;
  if (ctx->debug_blocks >= 1 && ctx->debug_blocks < blocks_ll) blocks_ll = ctx->debug_blocks;
  if (blocks_ll > blocks_needed) blocks_ll = blocks_needed;
  // plateau rings: MAX_PAST doubles per resident segment (the context's scratch is sized for the fullest grid)
  if (static_cast<size_t>(blocks_ll) * kSegs * MI355_LBFGS_MAX_PAST > ctx->scratch_cap)
    return fail(MI355_ERR_INVALID_ARGUMENT, "resident grid larger than the context's plateau-ring scratch");
  args.scratch = ctx->scratch_dev;
  args.next_problem = ctx->queue_dev;
  HIP_TRY(hipMemsetAsync(ctx->queue_dev, 0, kQueueWords * sizeof(unsigned long long), stream));
  HIP_TRY(hipEventRecord(ctx->ev_start, stream));
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks_ll)), dim3(kWave), lds, stream, args, cfg);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ev_stop, stream));
  ctx->timed = true;
  ctx->last_W = W;
  ctx->last_E = E;
  ctx->last_blocks = static_cast<int>(blocks_ll);
  ctx->last_threads = kWave;
  ctx->last_lds = lds;
  ctx->last_mr = 0;
  ctx->last_variant = MI355_KERNEL_GENERAL;
  ctx->last_arith = MI355_ARITH_EXACT;
  return MI355_OK;
}

}  // namespace mi355
