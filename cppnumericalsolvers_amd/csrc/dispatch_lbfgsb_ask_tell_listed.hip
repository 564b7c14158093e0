// dispatch_lbfgsb_ask_tell_listed.hip — the step kernel of a COMPACTED mi355_lbfgsb_ask_tell handle
// (lbfgsb_ask_tell_kernel.hpp, listed_step_kernel) at every (coordinates per lane, history capacity) of
// dispatch_lbfgsb_ask_tell.hip: the same step on the problems of the handle's list, the caller's arrays indexed by the
// place in the list, the state, the scalars and the boxes by problem.  A unit of its own, so that the kernels of a handle
// that is never compacted are built exactly as before.
#define MI355_DISPATCH_TU 1
#define MI355_ASK_TELL_LISTED_TU 1
#include "ask_tell_host.hpp"
#include "lbfgsb_ask_tell_kernel.hpp"

namespace mi355 {
namespace {

template <int E, int M>
int launch_step(mi355_lbfgs_ctx* ctx, const ask_tell_box::Args& args, const long long* ids, long long listed,
                hipStream_t stream) {
  constexpr int W = ask_tell_box::kLanes;
  if (args.n > W * E || args.m > M) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the kernel does not cover n / m");
  const int lds = (kWave / W) * lbfgsb_lds_doubles_per_problem<M>(W * E, 0) * static_cast<int>(sizeof(double));
  ask_tell_box::Args rows = args;  // (the kernel reads the length of the list from B)
  rows.B = listed;
  return launch_ask_tell_rows<W, E>(ctx, ask_tell_box::listed_step_kernel<E, M>, lds, lds, listed, rows, stream, ids);
}

template <int E>
int by_capacity(mi355_lbfgs_ctx* ctx, const ask_tell_box::Args& args, const long long* ids, long long listed,
                hipStream_t stream) {
  if (ask_tell_box_capacity(args.m) == 5) return launch_step<E, 5>(ctx, args, ids, listed, stream);
  return launch_step<E, 8>(ctx, args, ids, listed, stream);
}

}  // namespace

int dispatch_ask_tell_box_listed_step(mi355_lbfgs_ctx* ctx, int E, const ask_tell_box::Args& args, const long long* ids,
                                      long long listed, hipStream_t stream) {
  if (!ids || listed > args.B) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: a listed step without a list");
  switch (E) {
    case 1: return by_capacity<1>(ctx, args, ids, listed, stream);
    case 2: return by_capacity<2>(ctx, args, ids, listed, stream);
    case 4: return by_capacity<4>(ctx, args, ids, listed, stream);
  }
  return fail(MI355_ERR_UNSUPPORTED, "internal: no Lbfgsb ask/tell kernel for this number of coordinates per lane");
}

}  // namespace mi355
