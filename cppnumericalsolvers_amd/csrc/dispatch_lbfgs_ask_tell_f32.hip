// dispatch_lbfgs_ask_tell_f32.hip — the kernels of the mi355_lbfgs_ask_tell_f32_* entry points
// (lbfgs_ask_tell_f32_kernel.hpp): the float step kernel in the six lane mappings of the float L-BFGS kernel (8, 16, 32,
// 64 lanes at one coordinate per lane, 64 lanes at two and four), the state initialisation and the result gather,
// launched through ask_tell_host.hpp.  No objective lives here: the caller evaluates.
#define MI355_DISPATCH_TU 1
#include "ask_tell_host.hpp"
#include "lbfgs_ask_tell_f32_kernel.hpp"

namespace mi355 {

int dispatch_ask_tell_f32_step(mi355_lbfgs_ctx* ctx, int W, int E, const ask_tell_f32::Args& args, hipStream_t stream) {
  return launch_for_lbfgs_mapping(W, E, "internal: no float ask/tell kernel for this (W, E)", [&](auto w, auto e) {
    constexpr int kW = decltype(w)::value, kE = decltype(e)::value;
    return launch_ask_tell_step<kW, kE>(ctx, ask_tell_f32::step_kernel<kW, kE>, 0, ask_tell_f32::step_lds_bytes<kW>(),
                                        args, stream);
  });
}

int dispatch_ask_tell_f32_init(const ask_tell_f32::Args& args, const float* x0, long long row, hipStream_t stream) {
  return launch_elementwise(ask_tell_common::init_kernel<float, ask_tell_f32::Scalars>, args.B * args.n, stream,
                            args.vectors, args.scalars, args.x_eval, x0, args.B, args.n, row);
}

int dispatch_ask_tell_f32_results(const ask_tell_f32::ResultArgs& args, hipStream_t stream) {
  return launch_elementwise(ask_tell_common::results_kernel<ask_tell_f32::ResultArgs, ask_tell_f32::CanonicalNan>,
                            args.B * args.n, stream, args);
}

}  // namespace mi355
