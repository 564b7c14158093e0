// dispatch_lbfgs_ask_tell_wide_listed.hip — the step kernel of a COMPACTED mi355_lbfgs_ask_tell_wide handle
// (lbfgs_ask_tell_wide_kernel.hpp, listed_step_kernel) for 256 and for 1024 threads per problem: the same step on the
// problems of the handle's list, the caller's arrays indexed by the place in the list.  Both kernels are entry points of
// one run_steps; the unit stays its own, beside its dense twin in a parallel build.
#define MI355_DISPATCH_TU 1
#include "lbfgs_ask_tell_wide_launch.hpp"
#include "ask_tell_compact_kernel.hpp"

namespace mi355 {

int dispatch_ask_tell_wide_listed_step(mi355_lbfgs_ctx* ctx, const ask_tell_wide::Args& args, const long long* ids,
                                       long long listed, hipStream_t stream) {
  if (!ids || listed > args.B) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: a listed step without a list");
  ask_tell_wide::Args rows = args;
  rows.B = listed;
  if (args.n >= kWideBigN)
    return launch_ask_tell_wide_rows<kWideThreadsBig>(ctx, ask_tell_wide::listed_step_kernel<kWideThreadsBig>, listed, rows,
                                                      stream, ids);
  return launch_ask_tell_wide_rows<kWideThreads>(ctx, ask_tell_wide::listed_step_kernel<kWideThreads>, listed, rows, stream,
                                                 ids);
}

// The compaction of this path's list (ask_tell_compact_kernel.hpp over this path's Scalars).  It stands here, with the
// kernels that run on the list it builds, and not in dispatch_ask_tell_compact.hip: that unit's kernels are the three
// wavefront paths', counted by tests/test_ask_tell_compact_cpu.py.
template <>
int dispatch_ask_tell_compact<double, ask_tell_wide::Scalars, ask_tell_wide::kPhaseFinished>(
    const ask_tell_compact::Args<double, ask_tell_wide::Scalars>& args, hipStream_t stream) {
  return ask_tell_compact::launch<double, ask_tell_wide::Scalars, ask_tell_wide::kPhaseFinished>(args, stream);
}

}  // namespace mi355
