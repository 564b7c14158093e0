// lbfgsb_ask_tell_config.hpp — what the entry points, the dispatch unit and the kernel of the ask/tell (reverse
// communication) L-BFGS-B path share (lbfgsb_ask_tell_kernel.hpp, dispatch_lbfgsb_ask_tell.hip, ask_tell_entry.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355_lbfgs.h"

struct mi355_lbfgs_ctx;

namespace mi355 {
namespace ask_tell_box {

constexpr int kLanes = 16;  // lanes per problem: one DPP row, the 2m <= 16 rows of the compact representation on it

// what a problem waits for between two step calls (Lbfgsb::Minimize, solver/lbfgsb.h:141-292, cut at its evaluations)
enum Phase : int {
  kPhaseFirst = 0,      // the evaluation at the start point (Minimize's prologue, :253)
  kPhaseClipStart = 1,  // the evaluation at clip(x) when the iterate the step starts from is infeasible (:148-153)
  kPhaseTrial = 2,      // the evaluation at the trial point wa - stp d of the running More-Thuente search (:189)
  kPhaseNoEval = 3,     // nothing: the search was refused at once (dginit >= 0); the next call finishes that iteration
  kPhaseCauchy = 4,     // the evaluation at the Cauchy point when no variable is free (:191-193)
  kPhaseClipNext = 5,   // the evaluation at clip(next.x) when the step left the box (:199-203)
  kPhaseFinished = 6,   // frozen: x_eval holds the returned x
};

// the evaluation a step call asks for: index of the handle's ask counters (mi355_lbfgsb_ask_tell_asks)
enum Ask : int {
  kAskClipStart = 0,
  kAskTrial = 1,
  kAskCauchy = 2,
  kAskClipNext = 3,
  kAskFirst = 4,   // counted by the state initialisation: every problem asks for it once
  kAskKinds = 5,
  kAskNothing = 5,   // still active, no evaluation wanted (kPhaseNoEval)
  kNotActive = -1,   // finished
};

// The scalars of one problem between two step calls, written by lane 0 of its segment: what lbfgsb_kernel.hpp keeps in
// registers across iterations, the progress record, the plateau ring, and the scalar state of mt_cvsrch at its evaluation
// (stmin / stmax included: lbfgs_ask_tell_config.hpp says why).
struct Scalars {
  double f;        // the value at the iterate the step started from, after the clip (vector X of the row)
  double f_state;  // the value at entry of the step, before the clip: Progress::Update's f_delta is taken against it
  double theta, last_pg;
  double x_delta, f_delta, gradient_norm;
  double stx, fx, dgx, sty, fy, dgy, stp, width, width1, finit, dginit, stmin, stmax;
  double past_f[MI355_LBFGS_MAX_PAST];  // plateau ring (stop.past > 0)
  int32_t phase, k, status, x_delta_violations;
  int32_t f_delta_violations, past_init, past_pos, brackt;
  int32_t stage1, infoc, ls_nfev, pad0;
  uint32_t nfev, sum_k, num_iterations, pad1;
};
static_assert(sizeof(Scalars) % 8 == 0, "rows of doubles follow");

// The state row of one problem, in doubles; P = 16 E is the padded width, m the history size of the solve, M the
// capacity of the kernel (5 or 8):
//   X  [P]     x of the iterate the step started from, after the clip (the search's wa; the returned x once finished)
//   G  [P]     the gradient there
//   D  [P]     the negated direction of the running search; the Cauchy point / the clipped point while that is asked
//   XS [P]     x at entry of the step, before the clip (Progress::Update's x_delta is taken against it)
//   Y  [m][P]  the chronological histories, oldest first
//   S  [m][P]
//   A  [M][M]  S^T Y, column major
//   SS [M][M]  S^T S
// The LU of MM is not kept: the call that computes a step re-assembles MM from A, SS and theta and factorises it — the
// operations and operands of the persistent kernel, hence its bits.
__host__ __device__ constexpr long long row_doubles(int m, int M, int P) {
  return static_cast<long long>(4 + 2 * m) * P + 2 * M * M;
}

struct Args {
  double* vectors;      // [B][row_doubles(m, M, P)]
  Scalars* scalars;     // [B]
  double* x_eval;       // [B][n]: the public evaluation buffer
  const double* f;      // [B]     the caller's values at x_eval
  const double* g;      // [B][n]  ... and gradients
  const double* lower;  // the handle's copy of the box: [n] (box_stride == 0) or [B][box_stride]
  const double* upper;
  long long box_stride;
  unsigned long long* active;  // zeroed before the launch: the problems that are not finished after it
  unsigned long long* asks;    // [kAskKinds], accumulated over the calls
  long long B;
  int n, m;
  mi355_lbfgs_stop stop;
};

struct ResultArgs {
  const double* vectors;
  const Scalars* scalars;
  double *x_out, *f_out, *g_out;  // any may be null
  mi355_lbfgs_progress* progress_out;
  long long B, row, row_p;  // doubles of a state row; of one padded vector
  int n;
};

// the state initialisation: x0 into x_eval and X, the caller's box (or the reference's default one) into the handle's
// copy — [n] for a shared box, [B][n] for rows
struct InitArgs {
  double* vectors;
  Scalars* scalars;
  double* x_eval;
  const double* x0;
  double* lower;              // the handle's copy
  double* upper;
  const double* lower_in;     // the caller's; both null: the default box lowest() .. max() (lbfgsb.h:124-129)
  const double* upper_in;
  long long box_stride_in;    // 0: one shared box of n
  unsigned long long* asks;
  int* nan_flag;              // set when a bound is NaN
  long long B, row;
  int n;
};

}  // namespace ask_tell_box

// dispatch_lbfgsb_ask_tell.hip: the step kernel at one, two and four coordinates per lane and capacity 5 and 8, the
// state initialisation and the result gather.
int dispatch_ask_tell_box_step(mi355_lbfgs_ctx* ctx, int E, const ask_tell_box::Args& args, hipStream_t stream);
int dispatch_ask_tell_box_init(const ask_tell_box::InitArgs& args, hipStream_t stream);
int dispatch_ask_tell_box_results(const ask_tell_box::ResultArgs& args, hipStream_t stream);
// dispatch_lbfgsb_ask_tell_listed.hip: the step kernel of a compacted handle at the same (E, capacity) — slot
// s < listed of x_eval / f / g belongs to problem ids[s]; the state, the scalars and the boxes stay by problem
int dispatch_ask_tell_box_listed_step(mi355_lbfgs_ctx* ctx, int E, const ask_tell_box::Args& args, const long long* ids,
                                      long long listed, hipStream_t stream);
constexpr int ask_tell_box_capacity(int m) { return m <= 5 ? 5 : 8; }

}  // namespace mi355
