// lbfgs_ask_tell_f32_config.hpp — what the entry points, the dispatch unit and the kernel of the float ask/tell (reverse
// communication) L-BFGS path share (lbfgs_ask_tell_f32_kernel.hpp, dispatch_lbfgs_ask_tell_f32.hip,
// ask_tell_entry.hip).  The phase words are those of lbfgs_ask_tell_config.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355_lbfgs.h"
#include "lbfgs_ask_tell_config.hpp"

struct mi355_lbfgs_ctx;

namespace mi355 {
namespace ask_tell_f32 {

using ask_tell::kPhaseFinished;
using ask_tell::kPhaseFirst;
using ask_tell::kPhaseNoEval;
using ask_tell::kPhaseTrial;

// The scalars of one problem between two step calls, written by lane 0 of its segment: what lbfgs_f32_kernel.hpp keeps
// in registers across iterations, its Progress fields, the plateau ring, s.y of every ring slot (the float kernel
// stores the denominator, not its reciprocal) and the scalar state of the float mt_cvsrch at its evaluation.
// stmin / stmax are kept too: without a bracket stmax is formed from the step BEFORE the clamp and the `stp = stx`
// fallback (more_thuente.h:179-195), so it cannot be re-formed from the step that was evaluated.
struct Scalars {
  float f, scaling_factor;
  float x_delta, f_delta, gradient_norm;
  float stx, fx, dgx, sty, fy, dgy, stp, width, width1, finit, dginit, stmin, stmax;
  float sy[MI355_LBFGS_MAX_M];          // s.y per ring slot
  float past_f[MI355_LBFGS_MAX_PAST];   // plateau ring (stop.past > 0)
  int32_t phase, mem_count, mem_pos, status;
  int32_t x_delta_violations, f_delta_violations, past_init, past_pos;
  int32_t brackt, stage1, infoc, ls_nfev;
  uint32_t nfev, sum_k, num_iterations, pad;
};
static_assert(sizeof(Scalars) == 296, "documented in include/mi355_lbfgs.h and DESIGN.md 4.14");

// vectors of one problem in the state row, each padded to P = W * E floats: x (the search's wa), g at it, d, then the
// S and Y rings of m slots.  The trial point is the fourth vector: it lives in x_eval.
__host__ __device__ constexpr long long row_floats(int m, int P) { return static_cast<long long>(3 + 2 * m) * P; }

struct Args {
  float* vectors;    // [B][row_floats(m, P)]
  Scalars* scalars;  // [B]
  float* x_eval;     // [B][n]: the public evaluation buffer
  const float* f;    // [B]     the caller's values at x_eval
  const float* g;    // [B][n]  ... and gradients
  unsigned long long* active;  // zeroed before the launch: the problems that are not finished after it
  long long B;
  int n, m;
  mi355_lbfgs_stop stop;
  // static_cast<float> of the stop record's thresholds, converted once
  float stop_x_delta, stop_f_delta, stop_gradient_norm, stop_past_delta;
};

struct ResultArgs {
  const float* vectors;
  const Scalars* scalars;
  float *x_out, *f_out, *g_out;  // any may be null
  mi355_lbfgs_progress* progress_out;
  long long B, row, row_p;  // floats of a state row; of one padded vector
  int n;
};

}  // namespace ask_tell_f32

// dispatch_lbfgs_ask_tell_f32.hip: the step kernel in the six mappings of the float kernel (W in {8, 16, 32, 64} at
// E = 1, W = 64 at E in {2, 4}), the state initialisation and the result gather.
int dispatch_ask_tell_f32_step(mi355_lbfgs_ctx* ctx, int W, int E, const ask_tell_f32::Args& args, hipStream_t stream);
int dispatch_ask_tell_f32_init(const ask_tell_f32::Args& args, const float* x0, long long row, hipStream_t stream);
int dispatch_ask_tell_f32_results(const ask_tell_f32::ResultArgs& args, hipStream_t stream);
// dispatch_lbfgs_ask_tell_f32_listed.hip: the step kernel of a compacted handle in the same six mappings — slot
// s < listed of x_eval / f / g belongs to problem ids[s]
int dispatch_ask_tell_f32_listed_step(mi355_lbfgs_ctx* ctx, int W, int E, const ask_tell_f32::Args& args,
                                      const long long* ids, long long listed, hipStream_t stream);

}  // namespace mi355
