// dispatch_lbfgsb_ask_tell.hip — the kernels of the mi355_lbfgsb_ask_tell_* entry points (lbfgsb_ask_tell_kernel.hpp):
// the step kernel at one, two and four coordinates per lane of the sixteen-lane segment (n <= 64) and history capacity
// 5 and 8 — the range of dispatch_lbfgsb_own_box.hip —, the state initialisation and the result gather, launched
// through ask_tell_host.hpp.  No objective lives here: the caller evaluates.
#define MI355_DISPATCH_TU 1
#include "ask_tell_host.hpp"
#include "lbfgsb_ask_tell_kernel.hpp"

namespace mi355 {
namespace ask_tell_box {

// x0 into the evaluation buffer and into vector X of the state row (whose padding and scalars the host has zeroed: phase
// "first evaluation pending"), so that results() before the first step returns the start point; the caller's box — or
// the reference's default one — into the handle's copy, with a flag raised for a NaN bound.  (Not a template, so it
// lives in the one unit that launches it, not in the kernel header the unit of the listed step kernels includes too.)
__global__ void init_kernel(const InitArgs a) {
  const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= a.B * a.n) return;
  const long long b = t / a.n;
  const int j = static_cast<int>(t - b * a.n);
  const double v = a.x0[t];
  a.x_eval[t] = v;
  a.vectors[b * a.row + j] = v;
  if (j == 0) a.scalars[b].status = MI355_STATUS_NOT_STARTED;
  if (t == 0) a.asks[kAskFirst] = static_cast<unsigned long long>(a.B);
  const bool rows = a.box_stride_in != 0;
  if (rows || b == 0) {
    double lo = -1.7976931348623157e308, hi = 1.7976931348623157e308;  // lowest() .. max() (lbfgsb.h:124-129)
    if (a.lower_in != nullptr) {
      lo = a.lower_in[b * a.box_stride_in + j];
      hi = a.upper_in[b * a.box_stride_in + j];
    }
    if (lo != lo || hi != hi) *a.nan_flag = 1;
    const long long at = rows ? t : j;
    a.lower[at] = lo;
    a.upper[at] = hi;
  }
}

}  // namespace ask_tell_box

int dispatch_ask_tell_box_step(mi355_lbfgs_ctx* ctx, int E, const ask_tell_box::Args& args, hipStream_t stream) {
  return launch_for_box_mapping(E, ask_tell_box_capacity(args.m), [&](auto e, auto m) {
    constexpr int kE = decltype(e)::value, kM = decltype(m)::value;
    if (args.n > ask_tell_box::kLanes * kE || args.m > kM)
      return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the kernel does not cover n / m");
    const int lds = ask_tell_box::step_lds_bytes<kE, kM>();
    return launch_ask_tell_step<ask_tell_box::kLanes, kE>(ctx, ask_tell_box::step_kernel<kE, kM>, lds, lds, args, stream);
  });
}

int dispatch_ask_tell_box_init(const ask_tell_box::InitArgs& args, hipStream_t stream) {
  return launch_elementwise(ask_tell_box::init_kernel, args.B * args.n, stream, args);
}

int dispatch_ask_tell_box_results(const ask_tell_box::ResultArgs& args, hipStream_t stream) {
  return launch_elementwise(ask_tell_common::results_kernel<ask_tell_box::ResultArgs, ask_tell_common::AsStored>,
                            args.B * args.n, stream, args);
}

}  // namespace mi355
