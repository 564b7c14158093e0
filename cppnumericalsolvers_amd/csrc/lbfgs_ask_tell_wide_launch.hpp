// lbfgs_ask_tell_wide_launch.hpp — the step launch the two dispatch units of the ask/tell path above n = 256 share
// (dispatch_lbfgs_ask_tell_wide.hip, dispatch_lbfgs_ask_tell_wide_listed.hip).
#pragma once
#include <cstdlib>

#include "ask_tell_host.hpp"
#include "ask_tell_kernel_common.hpp"
#include "lbfgs_ask_tell_wide_kernel.hpp"

namespace mi355 {

// kern: a step kernel of T threads per workgroup, one problem per workgroup, taking ask_tell_wide::Args (and, listed,
// the list after them: `more`).  A grid-stride loop over `rows` rows of the caller's arrays: as many workgroups as the
// chip holds (occupancy x CUs), as the rows need, or as MI355_DEBUG_SOLVE_BLOCKS allows.  The direction's home during
// the recursion is dynamic LDS while n <= MI355_WIDE_LDS_MAX_N (default 4096; 0: never), launch_wide's switch.
template <int T, class Kernel, class... More>
int launch_ask_tell_wide_rows(mi355_lbfgs_ctx* ctx, Kernel kern, long long rows, ask_tell_wide::Args args,
                              hipStream_t stream, const More&... more) {
  if (args.n <= MI355_LBFGS_MAX_N || args.m > kWideMaxM)
    return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the wide ask/tell step outside its range");
  if ((args.n >= kWideBigN) != (T == kWideThreadsBig))
    return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the workgroup size does not follow n");
  if (rows < 1 || rows > args.B) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the rows of a step do not fit the batch");
  int lds_max_n = 4096;
  if (const char* v = std::getenv("MI355_WIDE_LDS_MAX_N")) lds_max_n = std::atoi(v);   // A/B switch (0 = never)
  args.d_in_lds = (args.n <= lds_max_n) ? 1 : 0;
  const int lds = args.d_in_lds ? static_cast<int>(ask_tell_wide::padded(args.n) * sizeof(double)) : 0;
  if (lds > 0)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, T, lds));
  if (per_cu < 1) per_cu = 1;
  long long blocks = static_cast<long long>(per_cu) * ctx->num_cus;
  if (ctx->debug_blocks >= 1 && ctx->debug_blocks < blocks) blocks = ctx->debug_blocks;
  if (blocks > rows) blocks = rows;
  HIP_TRY(hipMemsetAsync(args.active, 0, sizeof(unsigned long long), stream));
  HIP_TRY(hipEventRecord(ctx->ev_start, stream));
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(T), lds, stream, args, more...);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ev_stop, stream));
  ctx->timed = true;
  ctx->last_W = T;
  ctx->last_E = 0;   // (as launch_wide reports its memory form)
  ctx->last_blocks = static_cast<int>(blocks);
  ctx->last_threads = T;
  ctx->last_lds = lds;
  ctx->last_mr = 0;
  ctx->last_variant = MI355_KERNEL_GENERAL;
  ctx->last_arith = MI355_ARITH_EXACT;
  return MI355_OK;
}

}  // namespace mi355
