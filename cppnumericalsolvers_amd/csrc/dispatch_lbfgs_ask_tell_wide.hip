// dispatch_lbfgs_ask_tell_wide.hip — the kernels of the mi355_lbfgs_ask_tell_wide_* entry points
// (lbfgs_ask_tell_wide_kernel.hpp): the step kernel for 256 and for 1024 threads per problem, the state initialisation and
// the result gather; and the workgroup evaluation of Rosenbrock and DiagQuadratic behind mi355_lbfgs_eval_batch above
// n = 256.  The step kernels evaluate no objective: the caller does.
#define MI355_DISPATCH_TU 1
#include "lbfgs_ask_tell_wide_launch.hpp"

namespace mi355 {

int dispatch_ask_tell_wide_step(mi355_lbfgs_ctx* ctx, const ask_tell_wide::Args& args, hipStream_t stream) {
  if (args.n >= kWideBigN)
    return launch_ask_tell_wide_rows<kWideThreadsBig>(ctx, ask_tell_wide::step_kernel<kWideThreadsBig>, args.B, args, stream);
  return launch_ask_tell_wide_rows<kWideThreads>(ctx, ask_tell_wide::step_kernel<kWideThreads>, args.B, args, stream);
}

int dispatch_ask_tell_wide_init(const ask_tell_wide::Args& args, const double* x0, long long row, hipStream_t stream) {
  return launch_elementwise(ask_tell_common::init_kernel<double, ask_tell_wide::Scalars>, args.B * args.n, stream,
                            args.vectors, args.scalars, args.x_eval, x0, args.B, args.n, row);
}

int dispatch_ask_tell_wide_results(const ask_tell_wide::ResultArgs& args, hipStream_t stream) {
  return launch_elementwise(ask_tell_common::results_kernel<ask_tell_wide::ResultArgs, ask_tell_common::AsStored>,
                            args.B * args.n, stream, args);
}

namespace {

// a workgroup per row while the chip has room, striding beyond
template <class Obj, int T>
int launch_wide_eval(mi355_lbfgs_ctx* ctx, const double* x, double* f_out, double* g_out, const double* obj_params,
                     long long B, int n, hipStream_t stream) {
  auto kern = ask_tell_wide::eval_kernel<Obj, T>;
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, T, 0));
  if (per_cu < 1) per_cu = 1;
  long long blocks = static_cast<long long>(per_cu) * ctx->num_cus;
  if (ctx->debug_blocks >= 1 && ctx->debug_blocks < blocks) blocks = ctx->debug_blocks;
  if (blocks > B) blocks = B;
  HIP_TRY(hipEventRecord(ctx->ev_start, stream));
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(T), 0, stream, x, f_out, g_out, obj_params, B, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ev_stop, stream));
  ctx->timed = true;
  ctx->last_W = T;
  ctx->last_E = 0;
  ctx->last_blocks = static_cast<int>(blocks);
  ctx->last_threads = T;
  ctx->last_lds = 0;
  ctx->last_mr = 0;
  ctx->last_variant = MI355_KERNEL_GENERAL;
  ctx->last_arith = MI355_ARITH_EXACT;
  return MI355_OK;
}

template <class Obj>
int wide_eval_objective(mi355_lbfgs_ctx* ctx, const double* x, double* f_out, double* g_out, const double* obj_params,
                        long long B, int n, hipStream_t stream) {
  if (n >= kWideBigN) return launch_wide_eval<Obj, kWideThreadsBig>(ctx, x, f_out, g_out, obj_params, B, n, stream);
  return launch_wide_eval<Obj, kWideThreads>(ctx, x, f_out, g_out, obj_params, B, n, stream);
}

}  // namespace

int dispatch_wide_eval(mi355_lbfgs_ctx* ctx, int objective, const double* x, double* f_out, double* g_out,
                       const double* obj_params, long long B, int n, hipStream_t stream) {
  switch (objective) {
    case MI355_OBJ_ROSENBROCK: return wide_eval_objective<RosenbrockWide>(ctx, x, f_out, g_out, obj_params, B, n, stream);
    case MI355_OBJ_DIAG_QUADRATIC:
      return wide_eval_objective<DiagQuadraticWide>(ctx, x, f_out, g_out, obj_params, B, n, stream);
  }
  return fail(MI355_ERR_UNSUPPORTED,
              "eval_batch at n > MI355_LBFGS_MAX_N is built for the Rosenbrock and DiagQuadratic objectives (a user "
              "objective's workgroup functor has solve entry points only)");
}

}  // namespace mi355
