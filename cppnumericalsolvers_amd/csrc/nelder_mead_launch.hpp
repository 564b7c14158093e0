// nelder_mead_launch.hpp — launch of the Nelder-Mead kernel (nelder_mead_kernel.hpp) for one functor type, shared by
// dispatch_nelder_mead.hip (built-in objectives) and the units _build.py generates for user functors.
#pragma once
#include "engine_internal.hpp"
#include "nelder_mead_kernel.hpp"

namespace mi355 {

template <int W, class Obj, bool FIRST>
int launch_nelder_mead_mode(mi355_lbfgs_ctx* ctx, SolveArgs args, const NelderMeadDeviceConfig& cfg, hipStream_t stream) {
  constexpr int kSegs = kWave / W;
  constexpr int kLdsLimit = 160 * 1024;
  if (args.n > W) return fail(MI355_ERR_INVALID_ARGUMENT, "NelderMead: lanes_per_problem must cover n");
  const int lds = kSegs * nelder_mead_lds_doubles(args.n, W) * static_cast<int>(sizeof(double));
  if (lds > kLdsLimit) return fail(MI355_ERR_INVALID_ARGUMENT, "NelderMead: the simplices do not fit LDS");
  auto kern = nelder_mead_kernel<W, Obj, FIRST>;
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

// value mode for every functor; first mode for those with a value-and-gradient entry (eval)
template <int W, class Obj>
int launch_nelder_mead(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const NelderMeadDeviceConfig& cfg, hipStream_t stream) {
  if (!cfg.first_mode) return launch_nelder_mead_mode<W, Obj, false>(ctx, args, cfg, stream);
  if constexpr (HasGradientEval<Obj>::value) {
    return launch_nelder_mead_mode<W, Obj, true>(ctx, args, cfg, stream);
  } else {
    return fail(MI355_ERR_INVALID_ARGUMENT, "NelderMead: this functor is value-only (no eval): value mode only");
  }
}

template <class Obj>
int launch_nelder_mead_w(mi355_lbfgs_ctx* ctx, int W, const SolveArgs& args, const NelderMeadDeviceConfig& cfg,
                         hipStream_t stream) {
  switch (W) {
    case 8: return launch_nelder_mead<8, Obj>(ctx, args, cfg, stream);
    case 16: return launch_nelder_mead<16, Obj>(ctx, args, cfg, stream);
    case 32: return launch_nelder_mead<32, Obj>(ctx, args, cfg, stream);
    case 64: return launch_nelder_mead<64, Obj>(ctx, args, cfg, stream);
  }
  return fail(MI355_ERR_INVALID_ARGUMENT, "NelderMead: lanes_per_problem must be 8, 16, 32 or 64");
}

}  // namespace mi355
