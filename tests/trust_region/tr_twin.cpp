// tr_twin.cpp — C interface of the CPU twin (tr_twin.hpp) for tests/tr_lib.py.
#include "tr_twin.hpp"

extern "C" int tr_twin_solve(int objective, int n, int64_t B, const double* params, const tr_stop* st,
                             double condition_stop, const tr_config* cfg, int order, int W, const double* x0,
                             double* x_out, double* f_out, double* g_out, tr_progress* prog) {
  if (n < 1 || n > W || (objective == kTrQuartic && n != 1)) return -1;
  const tr_twin::Objective obj{objective, n, params};
  for (int64_t b = 0; b < B; ++b)
    tr_twin::solve_one(obj, static_cast<tr_twin::Order>(order), W, *st, condition_stop, *cfg, x0 + b * n, x_out + b * n,
                       f_out + b, g_out + b * n, prog + b);
  return 0;
}

// The same solve with the twin's counters (may be null) and, mutation = 1, tr_twin::kProductWalksColumn planted (tests:
// the recorded asymmetric inputs must notice it).
extern "C" int tr_twin_solve_ex(int objective, int n, int64_t B, const double* params, const tr_stop* st,
                                double condition_stop, const tr_config* cfg, int order, int W, int mutation,
                                const double* x0, double* x_out, double* f_out, double* g_out, tr_progress* prog,
                                tr_counters* counters) {
  if (n < 1 || n > W || (objective == kTrQuartic && n != 1) || mutation < 0 || mutation > 1) return -1;
  const tr_twin::Objective obj{objective, n, params};
  for (int64_t b = 0; b < B; ++b)
    tr_twin::solve_one(obj, static_cast<tr_twin::Order>(order), W, *st, condition_stop, *cfg, x0 + b * n, x_out + b * n,
                       f_out + b, g_out + b * n, prog + b, counters ? counters + b : nullptr,
                       static_cast<tr_twin::Mutation>(mutation));
  return 0;
}

// The twin's ||A||_F ||A^-1||_F on a caller-given matrix (n x n, column major), so that a test can hold it against a
// high-precision elimination (tests/test_dense_lu_mpmath.py).
extern "C" double tr_twin_condition(const double* A, int n) {
  return tr_twin::condition(std::vector<double>(A, A + n * n), n);
}
