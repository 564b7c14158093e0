// lbfgs_f32_config.hpp — what the entry points, the dispatch unit and the kernel of the native fp32 L-BFGS path share
// (lbfgs_f32_kernel.hpp, dispatch_lbfgs_f32.hip, solver_entry.hip, host_pipeline.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "lbfgs_kernel.hpp"

struct mi355_lbfgs_ctx;

namespace mi355 {
namespace f32 {

// What the float path adds to SolveArgs (whose B, n, m, stop counts and flags, count_dev, problem_map, next_problem,
// scratch and progress_out it reads; the double array pointers of SolveArgs are null here).
struct LbfgsF32Args {
  const float* x0;
  float* x_out;
  float* f_out;
  float* g_out;             // may be null
  const float* obj_params;  // device: the objective's parameters, converted to float on upload
  // static_cast<float> of the stop record's thresholds
  float stop_x_delta, stop_f_delta, stop_gradient_norm, stop_past_delta;
};

// floats of LDS per segment: the (s, y) ring, then s.y and alpha per slot
__host__ __device__ constexpr int lds_floats_per_problem(int m, int WE) { return 2 * m * WE + 2 * m; }

}  // namespace f32

// dispatch_lbfgs_f32.hip: the 12 solve kernels (W in {8, 16, 32, 64} at E = 1, W = 64 at E in {2, 4}; Rosenbrock and
// DiagQuadratic) and the 12 evaluation kernels.  The entry points have refused everything else.
int dispatch_lbfgs_f32(mi355_lbfgs_ctx* ctx, int W, int E, int objective, const SolveArgs& args,
                       const f32::LbfgsF32Args& fargs, hipStream_t stream);
int dispatch_eval_f32(int W, int E, int objective, const float* x, float* f_out, float* g_out, const float* params,
                      long long B, int n, hipStream_t stream);

}  // namespace mi355
