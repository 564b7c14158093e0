// ask_tell_kernel_common.hpp — the two element-wise kernels the ask/tell paths share (lbfgs_ask_tell_kernel.hpp,
// lbfgs_ask_tell_f32_kernel.hpp, lbfgsb_ask_tell_kernel.hpp): the state initialisation of the two Lbfgs paths and the
// result gather of all three.  One thread per element of [B][n].
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mi355_lbfgs.h"

namespace mi355 {
namespace ask_tell_common {

// x0 into the evaluation buffer and into the state row (whose padding and scalars the host has zeroed: phase
// "first evaluation pending"), so that results() before the first step returns the start point
template <class Scalar, class Scalars>
__global__ void init_kernel(Scalar* vectors, Scalars* scalars, Scalar* x_eval, const Scalar* x0, long long B, int n,
                            long long row) {
  const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= B * n) return;
  const long long b = t / n;
  const int j = static_cast<int>(t - b * n);
  const Scalar v = x0[t];
  x_eval[t] = v;
  vectors[b * row + j] = v;
  if (j == 0) scalars[b].status = MI355_STATUS_NOT_STARTED;
}

// how the double paths finish a value of the results: as it is
struct AsStored {
  __device__ static double value(double v) { return v; }
  __device__ static double widened(double v) { return v; }
};

// x, f, g and the progress record as the path's persistent kernel returns them.  Finish::value() is applied to what
// goes out in the path's scalar type, Finish::widened() to the three doubles of the progress record.
template <class ResultArgs, class Finish>
__global__ void results_kernel(const ResultArgs r) {
  const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= r.B * r.n) return;
  const long long b = t / r.n;
  const int j = static_cast<int>(t - b * r.n);
  const auto* const vec = r.vectors + b * r.row;
  if (r.x_out) r.x_out[t] = Finish::value(vec[j]);
  if (r.g_out) r.g_out[t] = Finish::value(vec[r.row_p + j]);
  if (j == 0) {
    const auto& s = r.scalars[b];
    if (r.f_out) r.f_out[b] = Finish::value(s.f);
    if (r.progress_out) {
      mi355_lbfgs_progress pr;
      pr.status = s.status;
      pr.num_iterations = s.num_iterations;
      pr.nfev = s.nfev;
      pr.sum_k = s.sum_k;
      pr.x_delta = Finish::widened(s.x_delta);
      pr.f_delta = Finish::widened(s.f_delta);
      pr.gradient_norm = Finish::widened(s.gradient_norm);
      r.progress_out[b] = pr;
    }
  }
}

}  // namespace ask_tell_common
}  // namespace mi355
