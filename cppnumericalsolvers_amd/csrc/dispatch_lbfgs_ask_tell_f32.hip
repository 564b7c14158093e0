// dispatch_lbfgs_ask_tell_f32.hip — the kernels of the mi355_lbfgs_ask_tell_f32_* entry points
// (lbfgs_ask_tell_f32_kernel.hpp): the float step kernel in the six lane mappings of the float L-BFGS kernel (8, 16, 32,
// 64 lanes at one coordinate per lane, 64 lanes at two and four), the state initialisation and the result gather.  No
// objective lives here: the caller evaluates.
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"
#include "lbfgs_ask_tell_f32_kernel.hpp"

namespace mi355 {
namespace {

template <int W, int E>
int launch_step(mi355_lbfgs_ctx* ctx, const ask_tell_f32::Args& args, hipStream_t stream) {
  constexpr int kSegs = kWave / W;
  if (args.n > W * E) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the lane mapping does not cover n");
  const auto kern = ask_tell_f32::step_kernel<W, E>;
  // a grid-stride loop over the batch: as many one-wavefront workgroups as the chip holds (or the batch needs)
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWave, 0));
  if (per_cu < 1) per_cu = 1;
  const long long blocks_needed = (args.B + kSegs - 1) / kSegs;
  long long blocks_ll = static_cast<long long>(per_cu) * ctx->num_cus;
  if (ctx->debug_blocks >= 1 && ctx->debug_blocks < blocks_ll) blocks_ll = ctx->debug_blocks;
  if (blocks_ll > blocks_needed) blocks_ll = blocks_needed;
  HIP_TRY(hipMemsetAsync(args.active, 0, sizeof(unsigned long long), stream));
  HIP_TRY(hipEventRecord(ctx->ev_start, stream));
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks_ll)), dim3(kWave), 0, stream, args);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ev_stop, stream));
  ctx->timed = true;
  ctx->last_W = W;
  ctx->last_E = E;
  ctx->last_blocks = static_cast<int>(blocks_ll);
  ctx->last_threads = kWave;
  ctx->last_lds = static_cast<int>(kSegs * 2 * MI355_LBFGS_MAX_M * sizeof(float));
  ctx->last_mr = 0;
  ctx->last_variant = MI355_KERNEL_GENERAL;
  ctx->last_arith = MI355_ARITH_EXACT;
  return MI355_OK;
}

}  // namespace

int dispatch_ask_tell_f32_step(mi355_lbfgs_ctx* ctx, int W, int E, const ask_tell_f32::Args& args, hipStream_t stream) {
  if (E == 1) {
    switch (W) {
      case 8: return launch_step<8, 1>(ctx, args, stream);
      case 16: return launch_step<16, 1>(ctx, args, stream);
      case 32: return launch_step<32, 1>(ctx, args, stream);
      case 64: return launch_step<64, 1>(ctx, args, stream);
    }
  }
  if (W == 64 && E == 2) return launch_step<64, 2>(ctx, args, stream);
  if (W == 64 && E == 4) return launch_step<64, 4>(ctx, args, stream);
  return fail(MI355_ERR_UNSUPPORTED, "internal: no float ask/tell kernel for this (W, E)");
}

int dispatch_ask_tell_f32_init(const ask_tell_f32::Args& args, const float* x0, long long row, hipStream_t stream) {
  const long long total = args.B * args.n;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(ask_tell_f32::init_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, args.vectors,
                     args.scalars, args.x_eval, x0, args.B, args.n, row);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}

int dispatch_ask_tell_f32_results(const ask_tell_f32::ResultArgs& args, hipStream_t stream) {
  const long long total = args.B * args.n;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(ask_tell_f32::results_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, args);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}

}  // namespace mi355
