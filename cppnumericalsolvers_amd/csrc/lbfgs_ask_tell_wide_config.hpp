// lbfgs_ask_tell_wide_config.hpp — what the entry points, the dispatch units and the kernel of the ask/tell L-BFGS path
// ABOVE n = 256 share (lbfgs_ask_tell_wide_kernel.hpp, dispatch_lbfgs_ask_tell_wide.hip and its listed twin,
// ask_tell_entry.hip), and the workgroup evaluation of the built-in objectives behind mi355_lbfgs_eval_batch there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mi355_lbfgs.h"

struct mi355_lbfgs_ctx;

namespace mi355 {
namespace ask_tell_wide {

// what a problem waits for between two step calls: the four phases of lbfgs_ask_tell_config.hpp, same values
enum Phase : int {
  kPhaseFirst = 0,     // the evaluation at the start point (Solver::Minimize's prologue)
  kPhaseTrial = 1,     // the evaluation at the trial point stp * (-d) + x of the running More-Thuente search
  kPhaseNoEval = 2,    // nothing: the search was refused at once (dginit >= 0); the next call finishes that iteration
  kPhaseFinished = 3,  // frozen: x_eval holds the returned x
};

// The scalars of one problem between two step calls, written by thread 0 of its workgroup: what lbfgs_wide_kernel keeps
// in registers across iterations (x . x, max |g_j| and max |x_j| travel with the iterate), s . y of every ring slot
// (its sy_mem), the plateau ring, and the 17 fields of MtSearch<double> under its names.
struct Scalars {
  double f, scaling_factor, xx_cur, gmax_cur, xmax_cur;
  double x_delta, f_delta, gradient_norm;
  double stx, fx, dgx, sty, fy, dgy, stp, width, width1, finit, dginit, stmin, stmax;
  double sy[MI355_LBFGS_MAX_M];         // s . y per ring slot (a pair with |s . y| < eps is skipped by the recursion)
  double past_f[MI355_LBFGS_MAX_PAST];  // plateau ring (stop.past > 0)
  int32_t phase, mem_count, mem_pos, status;
  int32_t x_delta_violations, f_delta_violations, past_init, past_pos;
  int32_t brackt, stage1, infoc, ls_nfev;
  uint32_t nfev, sum_k, num_iterations, pad;
};
static_assert(sizeof(Scalars) % 8 == 0, "rows of doubles follow");

// vectors of one problem in the state row, each padded to np = n rounded up to even (16-byte starts): x, g at it, d,
// then the S and Y rings of m slots.  The trial point is the fourth vector: it lives in x_eval.
__host__ __device__ constexpr long long padded(int n) { return (static_cast<long long>(n) + 1) & ~1LL; }
__host__ __device__ constexpr long long row_doubles(int m, long long np) { return (3 + 2LL * m) * np; }

struct Args {
  double* vectors;   // [B][row_doubles(m, np)]
  Scalars* scalars;  // [B]
  double* x_eval;    // [B][n]: the public evaluation buffer
  const double* f;   // [rows]     the caller's values at x_eval
  const double* g;   // [rows][n]  ... and gradients
  unsigned long long* active;  // zeroed before the launch: the problems that are not finished after it
  long long B;       // rows of this call: the batch, or the length of the list
  int n, m;
  mi355_lbfgs_stop stop;
  int d_in_lds;      // 1: the launch carries np doubles of dynamic LDS, the direction's home during the recursion
};

struct ResultArgs {
  const double* vectors;
  const Scalars* scalars;
  double *x_out, *f_out, *g_out;  // any may be null
  mi355_lbfgs_progress* progress_out;
  long long B, row, row_p;  // doubles of a state row; of one padded vector
  int n;
};

}  // namespace ask_tell_wide

// dispatch_lbfgs_ask_tell_wide.hip: the step kernel for 256 and 1024 threads per problem, the state initialisation and the
// result gather
int dispatch_ask_tell_wide_step(mi355_lbfgs_ctx* ctx, const ask_tell_wide::Args& args, hipStream_t stream);
int dispatch_ask_tell_wide_init(const ask_tell_wide::Args& args, const double* x0, long long row, hipStream_t stream);
int dispatch_ask_tell_wide_results(const ask_tell_wide::ResultArgs& args, hipStream_t stream);
// dispatch_lbfgs_ask_tell_wide_listed.hip: the step kernel of a compacted handle — slot s < listed of x_eval / f / g
// belongs to problem ids[s]
int dispatch_ask_tell_wide_listed_step(mi355_lbfgs_ctx* ctx, const ask_tell_wide::Args& args, const long long* ids,
                                       long long listed, hipStream_t stream);
// ... and, in the first unit, one evaluation per row at n > MI355_LBFGS_MAX_N with the workgroup functors of
// lbfgs_wide_kernel.hpp (Rosenbrock, DiagQuadratic): the f and g bits of the persistent kernel's evaluations
int dispatch_wide_eval(mi355_lbfgs_ctx* ctx, int objective, const double* x, double* f_out, double* g_out,
                       const double* obj_params, long long B, int n, hipStream_t stream);

}  // namespace mi355
