// dispatch_lbfgs_f32.hip — the kernels of mi355_lbfgs_minimize_batch_f32 and mi355_lbfgs_eval_batch_f32
// (lbfgs_f32_kernel.hpp): the six lane mappings of the first-order kernels (8, 16, 32, 64 lanes at one coordinate per
// lane, 64 lanes at two and four) on the float Rosenbrock and DiagQuadratic functors: 12 solve and 12 evaluation kernels.
#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"
#include "lbfgs_f32_kernel.hpp"
#include "solver_launch.hpp"

namespace mi355 {
namespace {

template <int W, int E, class Obj>
int launch_lbfgs_f32(mi355_lbfgs_ctx* ctx, const SolveArgs& args, const f32::LbfgsF32Args& fargs, hipStream_t stream) {
  constexpr int kSegs = kWave / W;
  constexpr int kLdsLimit = 160 * 1024;
  const int lds = kSegs * f32::lds_floats_per_problem(args.m, W * E) * static_cast<int>(sizeof(float));
  if (lds > kLdsLimit) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the float history ring does not fit LDS");
  return launch_persistent_solver<W, E>(ctx, f32::lbfgs_f32_kernel<W, E, Obj>, lds, args, fargs, stream);
}

template <int W, int E, class Obj>
int launch_eval_f32(const float* x, float* f_out, float* g_out, const float* params, long long B, int n,
                    hipStream_t stream) {
  constexpr int kSegs = kWave / W;
  const long long blocks = (B + kSegs - 1) / kSegs;
  hipLaunchKernelGGL((f32::eval_f32_kernel<W, E, Obj>), dim3(static_cast<unsigned>(blocks)), dim3(kWave), 0, stream, x,
                     f_out, g_out, params, B, n);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}

struct RosenbrockOf {
  template <int E>
  using type = f32::RosenbrockObjective;
};
struct DiagQuadraticOf {
  template <int E>
  using type = f32::DiagQuadraticObjective<E>;
};

// call(std::integral_constant<int, W>, std::integral_constant<int, E>) for one of the six built mappings
template <class Call>
int for_mapping(int W, int E, Call call) {
  using std::integral_constant;
  if (E == 1) {
    switch (W) {
      case 8: return call(integral_constant<int, 8>(), integral_constant<int, 1>());
      case 16: return call(integral_constant<int, 16>(), integral_constant<int, 1>());
      case 32: return call(integral_constant<int, 32>(), integral_constant<int, 1>());
      case 64: return call(integral_constant<int, 64>(), integral_constant<int, 1>());
    }
  }
  if (W == 64 && E == 2) return call(integral_constant<int, 64>(), integral_constant<int, 2>());
  if (W == 64 && E == 4) return call(integral_constant<int, 64>(), integral_constant<int, 4>());
  return fail(MI355_ERR_UNSUPPORTED, "internal: no float L-BFGS kernel for this (W, E)");
}

}  // namespace

int dispatch_lbfgs_f32(mi355_lbfgs_ctx* ctx, int W, int E, int objective, const SolveArgs& args,
                       const f32::LbfgsF32Args& fargs, hipStream_t stream) {
  if (objective == MI355_OBJ_ROSENBROCK)
    return for_mapping(W, E, [&](auto w, auto e) {
      return launch_lbfgs_f32<decltype(w)::value, decltype(e)::value, RosenbrockOf::type<decltype(e)::value>>(ctx, args, fargs, stream);
    });
  if (objective == MI355_OBJ_DIAG_QUADRATIC)
    return for_mapping(W, E, [&](auto w, auto e) {
      return launch_lbfgs_f32<decltype(w)::value, decltype(e)::value, DiagQuadraticOf::type<decltype(e)::value>>(ctx, args, fargs, stream);
    });
  return fail(MI355_ERR_UNSUPPORTED, "internal: no float L-BFGS kernel for this objective");
}

int dispatch_eval_f32(int W, int E, int objective, const float* x, float* f_out, float* g_out, const float* params,
                      long long B, int n, hipStream_t stream) {
  if (objective == MI355_OBJ_ROSENBROCK)
    return for_mapping(W, E, [&](auto w, auto e) {
      return launch_eval_f32<decltype(w)::value, decltype(e)::value, RosenbrockOf::type<decltype(e)::value>>(x, f_out, g_out, params, B, n, stream);
    });
  if (objective == MI355_OBJ_DIAG_QUADRATIC)
    return for_mapping(W, E, [&](auto w, auto e) {
      return launch_eval_f32<decltype(w)::value, decltype(e)::value, DiagQuadraticOf::type<decltype(e)::value>>(x, f_out, g_out, params, B, n, stream);
    });
  return fail(MI355_ERR_UNSUPPORTED, "internal: no float evaluation kernel for this objective");
}

}  // namespace mi355
