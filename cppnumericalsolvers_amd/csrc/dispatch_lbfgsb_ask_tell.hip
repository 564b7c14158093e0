// dispatch_lbfgsb_ask_tell.hip — the kernels of the mi355_lbfgsb_ask_tell_* entry points (lbfgsb_ask_tell_kernel.hpp):
// the step kernel at one, two and four coordinates per lane of the sixteen-lane segment (n <= 64) and history capacity
// 5 and 8 — the range of dispatch_lbfgsb_own_box.hip —, the state initialisation and the result gather.  No objective
// lives here: the caller evaluates.
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"
#include "lbfgsb_ask_tell_kernel.hpp"

namespace mi355 {
namespace {

template <int E, int M>
int launch_step(mi355_lbfgs_ctx* ctx, const ask_tell_box::Args& args, hipStream_t stream) {
  constexpr int W = ask_tell_box::kLanes;
  constexpr int kSegs = kWave / W;
  if (args.n > W * E || args.m > M) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the kernel does not cover n / m");
  const int lds = kSegs * lbfgsb_lds_doubles_per_problem<M>(W * E, 0) * static_cast<int>(sizeof(double));
  const auto kern = ask_tell_box::step_kernel<E, M>;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  // a grid-stride loop over the batch: as many one-wavefront workgroups as the chip holds (or the batch needs)
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWave, lds));
  if (per_cu < 1) per_cu = 1;
  const long long blocks_needed = (args.B + kSegs - 1) / kSegs;
  long long blocks_ll = static_cast<long long>(per_cu) * ctx->num_cus;
  if (ctx->debug_blocks >= 1 && ctx->debug_blocks < blocks_ll) blocks_ll = ctx->debug_blocks;
  if (blocks_ll > blocks_needed) blocks_ll = blocks_needed;
  HIP_TRY(hipMemsetAsync(args.active, 0, sizeof(unsigned long long), stream));
  HIP_TRY(hipEventRecord(ctx->ev_start, stream));
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks_ll)), dim3(kWave), lds, stream, args);
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

template <int E>
int by_capacity(mi355_lbfgs_ctx* ctx, const ask_tell_box::Args& args, hipStream_t stream) {
  if (ask_tell_box_capacity(args.m) == 5) return launch_step<E, 5>(ctx, args, stream);
  return launch_step<E, 8>(ctx, args, stream);
}

}  // namespace

int dispatch_ask_tell_box_step(mi355_lbfgs_ctx* ctx, int E, const ask_tell_box::Args& args, hipStream_t stream) {
  switch (E) {
    case 1: return by_capacity<1>(ctx, args, stream);
    case 2: return by_capacity<2>(ctx, args, stream);
    case 4: return by_capacity<4>(ctx, args, stream);
  }
  return fail(MI355_ERR_UNSUPPORTED, "internal: no Lbfgsb ask/tell kernel for this number of coordinates per lane");
}

int dispatch_ask_tell_box_init(const ask_tell_box::InitArgs& args, hipStream_t stream) {
  const long long total = args.B * args.n;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(ask_tell_box::init_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, args);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}

int dispatch_ask_tell_box_results(const ask_tell_box::ResultArgs& args, hipStream_t stream) {
  const long long total = args.B * args.n;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(ask_tell_box::results_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, args);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}

}  // namespace mi355
