// progress_device.hpp — the stopping tests of Progress::Update (solver/progress.h:212-317) for one problem on its
// segment, as a function for the solve kernels built on solver_driver.hpp, whose SolveProgress::update is the caller: it
// forms num_iterations, f_delta, x_delta and gradient_norm (:188-195); the kernel applies the condition_hessian test
// (:318-325) after it, since how H is obtained differs between the solvers.  lbfgs_kernel.hpp keeps its inline statement
// of the same tests: calling this function from it compiled to the same arithmetic but changed the scalar-register
// spills of several of its kernels (scripts/kernel_resources.py), whose budgets stay as they are.
#pragma once
#include "../../include/mi355_lbfgs.h"
#include "more_thuente_device.hpp"
#include "wave_primitives.hpp"

namespace mi355 {

// Running state of the tests between iterations (reset at the start of a solve).
// Returns MI355_STATUS_CONTINUE or the status of the first test that fires.
//   xinf_bound  running upper bound on ||x||_inf: the relative gradient test only computes ||x||_inf when even the bound
//               would let it fire (and then tightens the bound to the exact value)
//   past_f      the plateau ring (stop.past > 0), LDS or global scratch, written by lane 0 of the segment
template <int W, int E>
__device__ __forceinline__ int progress_stop_tests(const mi355_lbfgs_stop& st, unsigned long long stop_num_iterations,
                                                   double stop_gradient_norm, unsigned num_iterations, double f,
                                                   double fprev, double x_delta, double f_delta, double gradient_norm,
                                                   double& xinf_bound, const double (&x)[E], int& x_delta_violations,
                                                   int& f_delta_violations, double* past_f, bool& past_init,
                                                   int& past_pos, int sl) {
  int status = MI355_STATUS_CONTINUE;
  bool decided = false;
  if ((stop_num_iterations > 0) && (num_iterations > stop_num_iterations)) {  // :212-216
    status = MI355_STATUS_ITERATION_LIMIT;
    decided = true;
  }
  if (!decided) {                                      // :254-262
    if ((st.x_delta > 0) && (x_delta < st.x_delta)) {
      x_delta_violations++;
      if (x_delta_violations >= st.x_delta_violations) {
        status = MI355_STATUS_X_DELTA_VIOLATION;
        decided = true;
      }
    } else {
      x_delta_violations = 0;
    }
  }
  if (!decided) {                                      // :263-277
    const double fscale =
        st.f_delta_relative ? dmax(dmax(__builtin_fabs(f), __builtin_fabs(fprev)), 1.0) : 1.0;
    if ((st.f_delta > 0) && (f_delta < st.f_delta * fscale)) {
      f_delta_violations++;
      if (f_delta_violations >= st.f_delta_violations) {
        status = MI355_STATUS_F_DELTA_VIOLATION;
        decided = true;
      }
    } else {
      f_delta_violations = 0;
    }
  }
  if (!decided && st.past > 0) {                       // :280-298
    const int p = st.past;
    if (!past_init) {
      if (sl < p) past_f[sl] = f;                      // ring lazily filled with current f
      past_init = true;
      past_pos = 0;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (static_cast<int>(num_iterations) > p) {
      const double pf = past_f[past_pos];
      const double rate = __builtin_fabs(pf - f) / dmax(1.0, __builtin_fabs(f));
      if (rate < st.past_delta) {
        status = MI355_STATUS_F_DELTA_VIOLATION;
        decided = true;
      }
    }
    if (!decided) {
      if (sl == 0) past_f[past_pos] = f;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      past_pos = (past_pos + 1 == p) ? 0 : past_pos + 1;
    }
  }
  if (!decided && stop_gradient_norm > 0) {            // :299-317
    if (st.gradient_norm_relative) {
      // scale = max(1, ||x||_inf) <= max(1, bound): if even the bound's threshold is not
      // reached the test cannot fire and ||x||_inf need not be computed.
      if (gradient_norm < stop_gradient_norm * dmax(1.0, xinf_bound)) {
        const double xinf = seg_amax<W, E>(x);
        xinf_bound = xinf;
        if (gradient_norm < stop_gradient_norm * dmax(1.0, xinf)) status = MI355_STATUS_GRADIENT_NORM_VIOLATION;
      }
    } else if (gradient_norm < stop_gradient_norm) {
      status = MI355_STATUS_GRADIENT_NORM_VIOLATION;
    }
  }
  return status;
}

}  // namespace mi355
