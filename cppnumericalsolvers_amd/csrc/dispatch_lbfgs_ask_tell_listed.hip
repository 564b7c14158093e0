// dispatch_lbfgs_ask_tell_listed.hip — the step kernel of a COMPACTED mi355_lbfgs_ask_tell handle
// (lbfgs_ask_tell_kernel.hpp, listed_step_kernel) in the six lane mappings of dispatch_lbfgs_ask_tell.hip: the same step
// on the problems of the handle's list, the caller's arrays indexed by the place in the list.  A unit of its own, so
// that the kernels of a handle that is never compacted are built exactly as before.
#define MI355_DISPATCH_TU 1
#include "ask_tell_host.hpp"
#include "lbfgs_ask_tell_kernel.hpp"

namespace mi355 {
namespace {

template <int W, int E>
int launch_step(mi355_lbfgs_ctx* ctx, const ask_tell::Args& args, const long long* ids, long long listed,
                hipStream_t stream) {
  constexpr int kLds = (kWave / W) * (2 * MI355_LBFGS_MAX_M + 1) * static_cast<int>(sizeof(double));
  ask_tell::Args rows = args;  // (the kernel reads the length of the list from B)
  rows.B = listed;
  return launch_ask_tell_rows<W, E>(ctx, ask_tell::listed_step_kernel<W, E>, 0, kLds, listed, rows, stream, ids);
}

}  // namespace

int dispatch_ask_tell_listed_step(mi355_lbfgs_ctx* ctx, int W, int E, const ask_tell::Args& args, const long long* ids,
                                  long long listed, hipStream_t stream) {
  if (!ids || listed > args.B) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: a listed step without a list");
  if (E == 1) {
    switch (W) {
      case 8: return launch_step<8, 1>(ctx, args, ids, listed, stream);
      case 16: return launch_step<16, 1>(ctx, args, ids, listed, stream);
      case 32: return launch_step<32, 1>(ctx, args, ids, listed, stream);
      case 64: return launch_step<64, 1>(ctx, args, ids, listed, stream);
    }
  }
  if (W == 64 && E == 2) return launch_step<64, 2>(ctx, args, ids, listed, stream);
  if (W == 64 && E == 4) return launch_step<64, 4>(ctx, args, ids, listed, stream);
  return fail(MI355_ERR_UNSUPPORTED, "internal: no ask/tell kernel for this (W, E)");
}

}  // namespace mi355
