// fo_twin.cpp — C interface of the CPU twin (fo_twin.hpp) for tests/fo_lib.py.
#include "fo_twin.hpp"

#include <memory>

namespace {
std::unique_ptr<oracle::Objective> make_objective(int objective, int n, const double* params) {
  if (objective == kFoRosenbrock) return std::make_unique<oracle::Rosenbrock>();
  if (objective == kFoDiagQuadratic) {
    auto q = std::make_unique<oracle::DiagQuadratic>();
    q->a.assign(params, params + n);
    q->c = params[n];
    return q;
  }
  if (objective == kFoQuartic) return std::make_unique<fo_twin::Quartic>();
  return nullptr;
}
}  // namespace

// width: W x E of the device order (a power of two >= n, at most 1024); ignored in reference order
extern "C" int fo_twin_solve(int method, int objective, int n, int64_t B, const double* params, const fo_stop* st,
                             const fo_config* cfg, int order, int width, const double* x0, double* x_out, double* f_out,
                             double* g_out, fo_progress* prog, fo_counters* counters) {
  if (n < 1 || n > width || width > 1024 || (width & (width - 1)) != 0) return -1;
  if (method != kFoGradientDescent && method != kFoConjugatedGradientDescent) return -1;
  const auto obj = make_objective(objective, n, params);
  if (!obj) return -1;
  for (int64_t b = 0; b < B; ++b)
    fo_twin::solve_one(method, *obj, n, static_cast<fo_twin::Order>(order), width, *st, *cfg, x0 + b * n, x_out + b * n,
                       f_out + b, g_out + b * n, prog + b, counters ? counters + b : nullptr);
  return 0;
}

// One solve (the first row of x0) with its per-iteration states; *count = the rows written (at most capacity).
extern "C" int fo_twin_trajectory(int method, int objective, int n, const double* params, const fo_stop* st,
                                  const fo_config* cfg, int order, int width, const double* x0, double* x_out,
                                  double* f_out, double* g_out, fo_progress* prog, int capacity, double* rows, double* xs,
                                  int* count) {
  if (n < 1 || n > width || width > 1024 || (width & (width - 1)) != 0) return -1;
  const auto obj = make_objective(objective, n, params);
  if (!obj) return -1;
  fo_twin::Trajectory t{capacity, rows, xs, 0};
  fo_twin::solve_one(method, *obj, n, static_cast<fo_twin::Order>(order), width, *st, *cfg, x0, x_out, f_out, g_out,
                     prog, nullptr, &t);
  *count = t.count;
  return 0;
}
