// f32_twin.cpp — C interface of the float L-BFGS twin (f32_twin.hpp) for tests/l32_lib.py.
#include "f32_twin.hpp"

namespace {
bool shape_ok(int objective, int n, int m, int order, int width) {
  if (objective != kL32Rosenbrock && objective != kL32DiagQuadratic) return false;
  if (n < 1 || m < 1 || m > 32) return false;
  if (order == f32_twin::kDeviceOrder && (n > width || width > 1024 || (width & (width - 1)) != 0)) return false;
  return order == f32_twin::kRefOrder || order == f32_twin::kDeviceOrder;
}
}  // namespace

// width: W x E of the device order (a power of two >= n); ignored in reference order
extern "C" int l32_twin_solve(int objective, int n, int m, int64_t B, const double* params, const l32_stop* st, int order,
                              int width, const float* x0, float* x_out, float* f_out, float* g_out, l32_progress* prog) {
  if (!shape_ok(objective, n, m, order, width)) return -1;
  for (int64_t b = 0; b < B; ++b)
    f32_twin::solve_one(objective, params, n, m, static_cast<f32_twin::Order>(order), width, *st, x0 + b * n,
                        x_out + b * n, f_out + b, g_out + b * n, prog + b);
  return 0;
}

// One solve (the first row of x0) with its per-iteration rows and iterates; *count = the rows written
extern "C" int l32_twin_trajectory(int objective, int n, int m, const double* params, const l32_stop* st, int order,
                                   int width, const float* x0, float* x_out, float* f_out, float* g_out,
                                   l32_progress* prog, int capacity, double* rows, float* xs, int* count) {
  if (!shape_ok(objective, n, m, order, width)) return -1;
  f32_twin::Trajectory t{capacity, rows, xs, 0};
  f32_twin::solve_one(objective, params, n, m, static_cast<f32_twin::Order>(order), width, *st, x0, x_out, f_out, g_out,
                      prog, &t);
  *count = t.count;
  return 0;
}

// One evaluation per row
extern "C" int l32_twin_eval(int objective, int n, int64_t B, const double* params, int order, int width, const float* x,
                             float* f_out, float* g_out) {
  if (!shape_ok(objective, n, 1, order, width)) return -1;
  for (int64_t b = 0; b < B; ++b)
    f_out[b] = f32_twin::eval_one(objective, params, n, static_cast<f32_twin::Order>(order), width, x + b * n, g_out + b * n);
  return 0;
}
