// nm_twin.cpp — C interface of the CPU twin (nm_twin.hpp) for tests/nm_lib.py.  traj (may be null) records problem 0.
#include "nm_twin.hpp"

extern "C" int nm_twin_solve(int objective, int n, int64_t B, const double* params, const nm_stop* st,
                             const nm_config* cfg, int order, int W, const double* x0, double* x_out, double* f_out,
                             double* g_out, nm_progress* prog, int32_t* tied, nm_trajectory* traj) {
  if (n < 1 || n > W) return -1;
  if (objective != kNmRosenbrock && objective != kNmDiagQuadratic && objective != kNmL1Quadratic) return -1;
  if (objective == kNmL1Quadratic && cfg->mode != 0) return -1;
  const nm_twin::Objective obj{objective, n, params};
  if (traj != nullptr) traj->count = 0;
  for (int64_t b = 0; b < B; ++b)
    nm_twin::solve_one(obj, static_cast<nm_twin::Order>(order), W, *st, *cfg, x0 + b * n, x_out + b * n, f_out + b,
                       g_out + b * n, prog + b, tied + b, b == 0 ? traj : nullptr);
  return 0;
}
