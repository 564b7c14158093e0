// dispatch_lbfgsb_ask_tell.hip — the kernels of the mi355_lbfgsb_ask_tell_* entry points (lbfgsb_ask_tell_kernel.hpp):
// the step kernel at one, two and four coordinates per lane of the sixteen-lane segment (n <= 64) and history capacity
// 5 and 8 — the range of dispatch_lbfgsb_own_box.hip —, the state initialisation and the result gather, launched
// through ask_tell_host.hpp.  No objective lives here: the caller evaluates.
#define MI355_DISPATCH_TU 1
#include "ask_tell_host.hpp"
#include "lbfgsb_ask_tell_kernel.hpp"

namespace mi355 {
namespace {

template <int E, int M>
int launch_step(mi355_lbfgs_ctx* ctx, const ask_tell_box::Args& args, hipStream_t stream) {
  constexpr int W = ask_tell_box::kLanes;
  if (args.n > W * E || args.m > M) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the kernel does not cover n / m");
  const int lds = (kWave / W) * lbfgsb_lds_doubles_per_problem<M>(W * E, 0) * static_cast<int>(sizeof(double));
  return launch_ask_tell_step<W, E>(ctx, ask_tell_box::step_kernel<E, M>, lds, lds, args, stream);
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
  return launch_elementwise(ask_tell_box::init_kernel, args.B * args.n, stream, args);
}

int dispatch_ask_tell_box_results(const ask_tell_box::ResultArgs& args, hipStream_t stream) {
  return launch_elementwise(ask_tell_common::results_kernel<ask_tell_box::ResultArgs, ask_tell_common::AsStored>,
                            args.B * args.n, stream, args);
}

}  // namespace mi355
