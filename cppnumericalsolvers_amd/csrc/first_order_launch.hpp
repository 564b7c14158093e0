// first_order_launch.hpp — launch of the first-order kernel (first_order_kernel.hpp) for one functor type, shared by
// dispatch_first_order.hip (built-in objectives) and the units _build.py generates for user functors.
#pragma once
#include "engine_internal.hpp"
#include "first_order_kernel.hpp"

namespace mi355 {

template <int W, int E, int Method, class Obj>
int launch_first_order(mi355_lbfgs_ctx* ctx, SolveArgs args, const FirstOrderDeviceConfig& cfg, hipStream_t stream) {
  constexpr int kSegs = kWave / W;
  if (args.n > W * E) return fail(MI355_ERR_INVALID_ARGUMENT, "first-order solver: the lane mapping must cover n");
  auto kern = first_order_kernel<W, E, Method, Obj>;
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWave, 0));
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
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks_ll)), dim3(kWave), 0, stream, args, cfg);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ev_stop, stream));
  ctx->timed = true;
  ctx->last_W = W;
  ctx->last_E = E;
  ctx->last_blocks = static_cast<int>(blocks_ll);
  ctx->last_threads = kWave;
  ctx->last_lds = 0;
  ctx->last_mr = 0;
  ctx->last_variant = MI355_KERNEL_GENERAL;
  ctx->last_arith = MI355_ARITH_EXACT;
  return MI355_OK;
}

// The six built mappings: 8, 16, 32, 64 lanes at one coordinate per lane, 64 lanes at two and four.  ObjOf<W, E>::type
// is the functor type of a mapping (DiagQuadraticObjective is a template over E).
template <int Method, template <int, int> class ObjOf>
int launch_first_order_we(mi355_lbfgs_ctx* ctx, int W, int E, const SolveArgs& args, const FirstOrderDeviceConfig& cfg,
                          hipStream_t stream) {
  if (E == 1) {
    switch (W) {
      case 8: return launch_first_order<8, 1, Method, typename ObjOf<8, 1>::type>(ctx, args, cfg, stream);
      case 16: return launch_first_order<16, 1, Method, typename ObjOf<16, 1>::type>(ctx, args, cfg, stream);
      case 32: return launch_first_order<32, 1, Method, typename ObjOf<32, 1>::type>(ctx, args, cfg, stream);
      case 64: return launch_first_order<64, 1, Method, typename ObjOf<64, 1>::type>(ctx, args, cfg, stream);
    }
  } else if (W == 64 && E == 2) {
    return launch_first_order<64, 2, Method, typename ObjOf<64, 2>::type>(ctx, args, cfg, stream);
  } else if (W == 64 && E == 4) {
    return launch_first_order<64, 4, Method, typename ObjOf<64, 4>::type>(ctx, args, cfg, stream);
  }
  return fail(MI355_ERR_INVALID_ARGUMENT,
              "first-order solver: the mapping must be 8, 16, 32 or 64 lanes at one coordinate per lane, or 64 lanes at "
              "two or four");
}

template <template <int, int> class ObjOf>
int launch_first_order_method(mi355_lbfgs_ctx* ctx, int method, int W, int E, const SolveArgs& args,
                              const FirstOrderDeviceConfig& cfg, hipStream_t stream) {
  if (method == kGradientDescent)
    return launch_first_order_we<kGradientDescent, ObjOf>(ctx, W, E, args, cfg, stream);
  return launch_first_order_we<kConjugatedGradientDescent, ObjOf>(ctx, W, E, args, cfg, stream);
}

}  // namespace mi355
