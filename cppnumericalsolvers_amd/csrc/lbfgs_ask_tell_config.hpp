// lbfgs_ask_tell_config.hpp — what the entry points, the dispatch unit and the kernel of the ask/tell (reverse
// communication) L-BFGS path share (lbfgs_ask_tell_kernel.hpp, dispatch_lbfgs_ask_tell.hip, ask_tell_entry.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355_lbfgs.h"

struct mi355_lbfgs_ctx;

namespace mi355 {
namespace ask_tell {

// what a problem waits for between two step calls
enum Phase : int {
  kPhaseFirst = 0,     // the evaluation at the start point (Solver::Minimize's prologue)
  kPhaseTrial = 1,     // the evaluation at the trial point wa - stp d of the running More-Thuente search
  kPhaseNoEval = 2,    // nothing: the search was refused at once (dginit >= 0); the next call finishes that iteration
  kPhaseFinished = 3,  // frozen: x_eval holds the returned x
};

// The scalars of one problem between two step calls, written by lane 0 of its segment: what lbfgs_kernel.hpp keeps in
// registers across iterations, SolveProgress, the plateau ring, and the scalar state of mt_cvsrch at its evaluation.
// stmin / stmax are kept too: without a bracket stmax is formed from the step BEFORE the clamp and the `stp = stx`
// fallback (more_thuente.h:179-195), so it cannot be re-formed from the step that was evaluated.
struct Scalars {
  double f, scaling_factor, xinf_bound;
  double x_delta, f_delta, gradient_norm;
  double stx, fx, dgx, sty, fy, dgy, stp, width, width1, finit, dginit, stmin, stmax;
  double rho[MI355_LBFGS_MAX_M];        // 1 / (s.y) per ring slot, 0 = a pair the reference skips
  double past_f[MI355_LBFGS_MAX_PAST];  // plateau ring (stop.past > 0)
  int32_t phase, mem_count, mem_pos, status;
  int32_t x_delta_violations, f_delta_violations, past_init, past_pos;
  int32_t brackt, stage1, infoc, ls_nfev;
  uint32_t nfev, sum_k, num_iterations, pad;
};
static_assert(sizeof(Scalars) % 8 == 0, "rows of doubles follow");

// vectors of one problem in the state row, each padded to P = W * E doubles: x (the search's wa), g at it, d, then the
// S and Y rings of m slots.  The trial point is the fourth vector: it lives in x_eval.
__host__ __device__ constexpr long long row_doubles(int m, int P) { return static_cast<long long>(3 + 2 * m) * P; }

struct Args {
  double* vectors;   // [B][row_doubles(m, P)]
  Scalars* scalars;  // [B]
  double* x_eval;    // [B][n]: the public evaluation buffer
  const double* f;   // [B]     the caller's values at x_eval (step), x0 (init)
  const double* g;   // [B][n]  ... and gradients
  unsigned long long* active;  // zeroed before the launch: the problems that are not finished after it
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

}  // namespace ask_tell

// dispatch_lbfgs_ask_tell.hip: the step kernel in the six mappings of the first-order kernels (W in {8, 16, 32, 64} at
// E = 1, W = 64 at E in {2, 4}), the state initialisation and the result gather.
int dispatch_ask_tell_step(mi355_lbfgs_ctx* ctx, int W, int E, const ask_tell::Args& args, hipStream_t stream);
int dispatch_ask_tell_init(const ask_tell::Args& args, const double* x0, long long row, hipStream_t stream);
int dispatch_ask_tell_results(const ask_tell::ResultArgs& args, hipStream_t stream);
// dispatch_lbfgs_ask_tell_listed.hip: the step kernel of a compacted handle in the same six mappings — slot s < listed
// of x_eval / f / g belongs to problem ids[s]
int dispatch_ask_tell_listed_step(mi355_lbfgs_ctx* ctx, int W, int E, const ask_tell::Args& args, const long long* ids,
                                  long long listed, hipStream_t stream);

}  // namespace mi355
