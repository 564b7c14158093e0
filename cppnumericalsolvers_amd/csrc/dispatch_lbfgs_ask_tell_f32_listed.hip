// dispatch_lbfgs_ask_tell_f32_listed.hip — the step kernel of a COMPACTED mi355_lbfgs_ask_tell_f32 handle
// (lbfgs_ask_tell_f32_kernel.hpp, listed_step_kernel) in the six lane mappings of dispatch_lbfgs_ask_tell_f32.hip: the
// same float step on the problems of the handle's list, the caller's arrays indexed by the place in the list.  Both
// kernels are entry points of one run_steps; the unit stays its own, beside its dense twin in a parallel build.
#define MI355_DISPATCH_TU 1
#include "ask_tell_host.hpp"
#include "lbfgs_ask_tell_f32_kernel.hpp"

namespace mi355 {

int dispatch_ask_tell_f32_listed_step(mi355_lbfgs_ctx* ctx, int W, int E, const ask_tell_f32::Args& args,
                                      const long long* ids, long long listed, hipStream_t stream) {
  return launch_for_lbfgs_mapping(W, E, "internal: no float ask/tell kernel for this (W, E)", [&](auto w, auto e) {
    constexpr int kW = decltype(w)::value, kE = decltype(e)::value;
    return launch_ask_tell_listed<kW, kE>(ctx, ask_tell_f32::listed_step_kernel<kW, kE>, 0,
                                          ask_tell_f32::step_lds_bytes<kW>(), args, ids, listed, stream);
  });
}

}  // namespace mi355
