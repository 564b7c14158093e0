// derivative_check_launch.hpp — launches of the derivative-check kernels (derivative_check_kernel.hpp) for one functor
// type, shared by dispatch_derivatives.hip (built-in objectives) and the units _build.py generates for user functors
// (derivatives=True).
#pragma once
#include "derivative_check_kernel.hpp"
#include "engine_internal.hpp"

namespace mi355 {

// one-shot grid: items / segments per wavefront, rounded up
inline int derivative_grid(long long items, int segs, unsigned* blocks) {
  const long long b = (items + segs - 1) / segs;
  if (b > 0x7fffffffLL) return fail(MI355_ERR_INVALID_ARGUMENT, "derivative check: the batch is too large for one grid");
  *blocks = static_cast<unsigned>(b);
  return MI355_OK;
}

// stands for a mapping a user functor's unit was not built for (_build.py, derivatives=dict(elems=...))
struct DerivativeNotBuilt {};

template <int W, int E, class Obj>
int launch_derivative_gradient(mi355_lbfgs_ctx*, const DerivativeArgs& args, hipStream_t stream) {
  constexpr int kSegs = kWave / W;
  if constexpr (std::is_same<Obj, DerivativeNotBuilt>::value) {
    return fail(MI355_ERR_UNSUPPORTED,
                "derivative check: this user objective's derivative kernels were not built for this many coordinates per "
                "lane (derivatives=dict(elems=...))");
  } else {
    if (args.n > W * E) return fail(MI355_ERR_INVALID_ARGUMENT, "derivative check: the lane mapping must cover n");
    if constexpr (!HasEval<Obj, W, E>::value) {
      if (args.grad_out != nullptr)
        return fail(MI355_ERR_UNSUPPORTED,
                    "derivative check: this functor has no eval (value-only): it has no analytic gradient to return or to "
                    "check; pass grad_out = NULL for the finite-difference gradient alone");
    }
    unsigned blocks = 0;
    const int rc = derivative_grid(args.B, kSegs, &blocks);
    if (rc != MI355_OK) return rc;
    hipLaunchKernelGGL((dv_gradient_kernel<W, E, Obj>), dim3(blocks), dim3(kWave), 0, stream, args);
    HIP_TRY(hipGetLastError());
    return MI355_OK;
  }
}

// phase: kDerivativeHessian (hess_full -> hess_out) or kDerivativeFiniteHessian (-> hess_fd_out); one coordinate per lane
template <int W, class Obj>
int launch_derivative_hessian(mi355_lbfgs_ctx*, int phase, const DerivativeArgs& args, hipStream_t stream) {
  constexpr int kSegs = kWave / W;
  constexpr int kLdsLimit = 160 * 1024;
  if (args.n > W) return fail(MI355_ERR_INVALID_ARGUMENT, "derivative check: lanes_per_problem must cover n for the Hessian");
  unsigned blocks = 0;
  if (phase == kDerivativeFiniteHessian) {
    const int rc = derivative_grid(args.B * args.n, kSegs, &blocks);
    if (rc != MI355_OK) return rc;
    hipLaunchKernelGGL((dv_finite_hessian_kernel<W, Obj>), dim3(blocks), dim3(kWave), 0, stream, args);
    HIP_TRY(hipGetLastError());
    return MI355_OK;
  }
  if constexpr (HasHessFull<Obj>::value) {
    const int lds = kSegs * args.n * args.n * static_cast<int>(sizeof(double));
    if (lds > kLdsLimit)
      return fail(MI355_ERR_INVALID_ARGUMENT, "derivative check: the Hessians of a wavefront's points do not fit LDS (160 KB)");
    const int rc = derivative_grid(args.B, kSegs, &blocks);
    if (rc != MI355_OK) return rc;
    auto kern = dv_hessian_kernel<W, Obj>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWave), lds, stream, args);
    HIP_TRY(hipGetLastError());
    return MI355_OK;
  } else {
    return fail(MI355_ERR_UNSUPPORTED,
                "derivative check: this functor has no hess_full: it has no analytic Hessian to return or to check; pass "
                "hess_out = NULL for the finite-difference Hessian alone");
  }
}

// The mappings: 8, 16, 32, 64 lanes at one coordinate per lane (gradient and Hessian), 64 lanes at two and four
// (gradient).  ObjOf<W, E>::type is the functor type of a mapping.
template <template <int, int> class ObjOf>
int launch_derivatives(mi355_lbfgs_ctx* ctx, int phase, int W, int E, const DerivativeArgs& args, hipStream_t stream) {
  if (phase == kDerivativeGradient) {
    if (E == 1) {
      switch (W) {
        case 8: return launch_derivative_gradient<8, 1, typename ObjOf<8, 1>::type>(ctx, args, stream);
        case 16: return launch_derivative_gradient<16, 1, typename ObjOf<16, 1>::type>(ctx, args, stream);
        case 32: return launch_derivative_gradient<32, 1, typename ObjOf<32, 1>::type>(ctx, args, stream);
        case 64: return launch_derivative_gradient<64, 1, typename ObjOf<64, 1>::type>(ctx, args, stream);
      }
    } else if (W == 64 && E == 2) {
      return launch_derivative_gradient<64, 2, typename ObjOf<64, 2>::type>(ctx, args, stream);
    } else if (W == 64 && E == 4) {
      return launch_derivative_gradient<64, 4, typename ObjOf<64, 4>::type>(ctx, args, stream);
    }
  } else if (E == 1) {
    switch (W) {
      case 8: return launch_derivative_hessian<8, typename ObjOf<8, 1>::type>(ctx, phase, args, stream);
      case 16: return launch_derivative_hessian<16, typename ObjOf<16, 1>::type>(ctx, phase, args, stream);
      case 32: return launch_derivative_hessian<32, typename ObjOf<32, 1>::type>(ctx, phase, args, stream);
      case 64: return launch_derivative_hessian<64, typename ObjOf<64, 1>::type>(ctx, phase, args, stream);
    }
  }
  return fail(MI355_ERR_INVALID_ARGUMENT,
              "derivative check: the mapping must be 8, 16, 32 or 64 lanes at one coordinate per lane, or (gradient only) "
              "64 lanes at two or four");
}

// what a functor type offers (the same for every mapping)
template <template <int, int> class ObjOf>
constexpr int derivative_capabilities() {
  using Obj = typename ObjOf<8, 1>::type;
  return (HasEval<Obj, 8, 1>::value ? kDerivativeHasEval : 0) | (HasHessFull<Obj>::value ? kDerivativeHasHessFull : 0);
}

}  // namespace mi355
