// newton_descent_launch.hpp — launch of the Newton-descent kernel (newton_descent_kernel.hpp) for one functor type, shared by
// dispatch_newton_descent.hip (built-in objectives) and the units _build.py generates for user functors.
#pragma once
#include "engine_internal.hpp"
#include "newton_descent_kernel.hpp"

namespace mi355 {

template <int W, class Obj>
int launch_newton_descent(mi355_lbfgs_ctx* ctx, SolveArgs args, const NewtonDescentDeviceConfig& cfg, hipStream_t stream) {
  constexpr int kSegs = kWave / W;
  constexpr int kLdsLimit = 160 * 1024;
  if (args.n > W) return fail(MI355_ERR_INVALID_ARGUMENT, "NewtonDescent: lanes_per_problem must cover n");
  const int lds = kSegs * newton_descent_lds_doubles(args.n, W, args.hessian_condition_stop > 0.0) *
                  static_cast<int>(sizeof(double));
  if (lds > kLdsLimit) return fail(MI355_ERR_INVALID_ARGUMENT, "NewtonDescent: the Hessians and their LU copies do not fit LDS");
  auto kern = newton_descent_kernel<W, Obj>;
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
  ctx->last_E = 1;
  ctx->last_blocks = static_cast<int>(blocks_ll);
  ctx->last_threads = kWave;
  ctx->last_lds = lds;
  ctx->last_mr = 0;
  ctx->last_variant = MI355_KERNEL_GENERAL;
  ctx->last_arith = MI355_ARITH_EXACT;
  return MI355_OK;
}

template <class Obj>
int launch_newton_descent_w(mi355_lbfgs_ctx* ctx, int W, const SolveArgs& args, const NewtonDescentDeviceConfig& cfg,
                          hipStream_t stream) {
  switch (W) {
    case 8: return launch_newton_descent<8, Obj>(ctx, args, cfg, stream);
    case 16: return launch_newton_descent<16, Obj>(ctx, args, cfg, stream);
    case 32: return launch_newton_descent<32, Obj>(ctx, args, cfg, stream);
    case 64: return launch_newton_descent<64, Obj>(ctx, args, cfg, stream);
  }
  return fail(MI355_ERR_INVALID_ARGUMENT, "NewtonDescent: lanes_per_problem must be 8, 16, 32 or 64");
}

}  // namespace mi355
