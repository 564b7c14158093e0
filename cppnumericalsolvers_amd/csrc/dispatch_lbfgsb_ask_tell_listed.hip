// dispatch_lbfgsb_ask_tell_listed.hip — the step kernel of a COMPACTED mi355_lbfgsb_ask_tell handle
// (lbfgsb_ask_tell_kernel.hpp, listed_step_kernel) at every (coordinates per lane, history capacity) of
// dispatch_lbfgsb_ask_tell.hip: the same step on the problems of the handle's list, the caller's arrays indexed by the
// place in the list, the state, the scalars and the boxes by problem.  Both kernels are entry points of one run_steps; a
// unit of its own, so that the two longest compiles of the library run side by side.
#define MI355_DISPATCH_TU 1
#include "ask_tell_host.hpp"
#include "lbfgsb_ask_tell_kernel.hpp"

namespace mi355 {

int dispatch_ask_tell_box_listed_step(mi355_lbfgs_ctx* ctx, int E, const ask_tell_box::Args& args, const long long* ids,
                                      long long listed, hipStream_t stream) {
  return launch_for_box_mapping(E, ask_tell_box_capacity(args.m), [&](auto e, auto m) {
    constexpr int kE = decltype(e)::value, kM = decltype(m)::value;
    if (args.n > ask_tell_box::kLanes * kE || args.m > kM)
      return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the kernel does not cover n / m");
    const int lds = ask_tell_box::step_lds_bytes<kE, kM>();
    return launch_ask_tell_listed<ask_tell_box::kLanes, kE>(ctx, ask_tell_box::listed_step_kernel<kE, kM>, lds, lds, args,
                                                            ids, listed, stream);
  });
}

}  // namespace mi355
