// dispatch_derivatives.hip — the kernels of mi355_check_derivatives_batch (derivative_check_kernel.hpp) on the built-in
// objectives without LDS data: Rosenbrock and DiagQuadratic, through their Hessian-carrying types.  User functors get
// their own units (_build.py, derivatives=True).  The compare kernel, which needs no functor, is launched from here too.
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"
#include "derivative_check_launch.hpp"

namespace mi355 {
namespace {
template <int W, int E>
struct RosenbrockOf {
  using type = RosenbrockConditionObjective;
};
template <int W, int E>
struct DiagQuadraticOf {
  using type = DiagQuadraticHessObjective<E>;
};
// every report starts as "nothing checked"
__global__ void dv_report_init_kernel(mi355_derivative_report* report, long long B) {
  const long long b = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b >= B) return;
  mi355_derivative_report r;
  r.gradient_ok = r.hessian_ok = -1;
  r.gradient_worst_index = r.hessian_worst_index = -1;
  r.nonfinite = 0;
  r.pad = 0;
  r.gradient_worst_excess = r.hessian_worst_excess = 0.0;
  report[b] = r;
}

}  // namespace

int derivative_capabilities_of(int objective) {
  switch (objective) {
    case MI355_OBJ_ROSENBROCK: return derivative_capabilities<RosenbrockOf>();
    case MI355_OBJ_DIAG_QUADRATIC: return derivative_capabilities<DiagQuadraticOf>();
  }
  int capabilities = 0;
  return user_solver(objective, kUserDerivatives, &capabilities) != nullptr ? capabilities : -1;
}

int dispatch_derivatives(mi355_lbfgs_ctx* ctx, int phase, int W, int E, int objective, const DerivativeArgs& args,
                         hipStream_t stream) {
  switch (objective) {
    case MI355_OBJ_ROSENBROCK: return launch_derivatives<RosenbrockOf>(ctx, phase, W, E, args, stream);
    case MI355_OBJ_DIAG_QUADRATIC: return launch_derivatives<DiagQuadraticOf>(ctx, phase, W, E, args, stream);
  }
  if (const auto fn = user_solver_fn<kUserDerivatives>(objective)) return fn(ctx, phase, W, E, args, stream);
  return fail(MI355_ERR_UNSUPPORTED, derivative_unsupported_message(objective));
}

const char* derivative_unsupported_message(int objective) {
  return objective >= MI355_OBJ_USER_FIRST
             ? "derivative check: this library holds no derivative kernel for this user objective (build it with "
               "derivatives=True)"
             : "the derivative check is built for objectives without LDS data: Rosenbrock, DiagQuadratic and user "
               "functors built with derivatives=True; not the ridge forms or the augmented-Lagrangian composite";
}

int derivative_report_init(mi355_derivative_report* report, long long B, hipStream_t stream) {
  const int threads = 256;
  const long long blocks = (B + threads - 1) / threads;
  if (blocks > 0x7fffffffLL) return fail(MI355_ERR_INVALID_ARGUMENT, "derivative check: the batch is too large for one grid");
  hipLaunchKernelGGL(dv_report_init_kernel, dim3(static_cast<unsigned>(blocks)), dim3(threads), 0, stream, report, B);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}

int derivative_compare(const DerivativeCompareArgs& args, bool hessian, hipStream_t stream) {
  if (args.B > 0x7fffffffLL) return fail(MI355_ERR_INVALID_ARGUMENT, "derivative check: the batch is too large for one grid");
  if (hessian) hipLaunchKernelGGL(dv_compare_kernel<true>, dim3(static_cast<unsigned>(args.B)), dim3(kWave), 0, stream, args);
  else hipLaunchKernelGGL(dv_compare_kernel<false>, dim3(static_cast<unsigned>(args.B)), dim3(kWave), 0, stream, args);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}

}  // namespace mi355
