// nd_twin.cpp — C interface of the CPU twin (nd_twin.hpp) for tests/nd_lib.py.
#include "nd_twin.hpp"

extern "C" int nd_twin_solve(int objective, int n, int64_t B, const double* params, const nd_stop* st,
                             double condition_stop, const nd_config* cfg, int order, int W, const double* x0,
                             double* x_out, double* f_out, double* g_out, nd_progress* prog, nd_counters* counters) {
  if (n < 1 || n > W) return -1;
  const nd_twin::Objective obj{objective, n, params};
  for (int64_t b = 0; b < B; ++b)
    nd_twin::solve_one(obj, static_cast<nd_twin::Order>(order), W, *st, condition_stop, *cfg, x0 + b * n, x_out + b * n,
                       f_out + b, g_out + b * n, prog + b, counters ? counters + b : nullptr);
  return 0;
}

// The same solve with one of nd_twin::Mutation's deliberate bugs planted (tests: the recorded inputs must notice it).
extern "C" int nd_twin_solve_mutated(int objective, int n, int64_t B, const double* params, const nd_stop* st,
                                     double condition_stop, const nd_config* cfg, int order, int W, int mutation,
                                     const double* x0, double* x_out, double* f_out, double* g_out, nd_progress* prog) {
  if (n < 1 || n > W || mutation < 0 || mutation > 2) return -1;
  const nd_twin::Objective obj{objective, n, params};
  for (int64_t b = 0; b < B; ++b)
    nd_twin::solve_one(obj, static_cast<nd_twin::Order>(order), W, *st, condition_stop, *cfg, x0 + b * n, x_out + b * n,
                       f_out + b, g_out + b * n, prog + b, nullptr, nullptr, static_cast<nd_twin::Mutation>(mutation));
  return 0;
}

// The twin's LU, solve and condition number on a caller-given matrix (n x n, column major), so that a test can hold
// them against a high-precision elimination (tests/test_dense_lu_mpmath.py).  lu_factor overwrites A with its LU.
extern "C" int nd_twin_lu_factor(double* A, int32_t* piv, int n) {
  if (n < 1 || n > kNdMaxN) return -1;
  std::vector<double> a(A, A + n * n);
  std::vector<int> p;
  nd_twin::lu_factor(a, p, n);
  for (int t = 0; t < n * n; ++t) A[t] = a[t];
  for (int k = 0; k < n; ++k) piv[k] = p[k];
  return 0;
}
extern "C" int nd_twin_lu_solve(const double* LU, const int32_t* piv, double* x, int n) {
  if (n < 1 || n > kNdMaxN) return -1;
  const std::vector<double> a(LU, LU + n * n);
  const std::vector<int> p(piv, piv + n);
  nd_twin::lu_solve(a, p, x, n);
  return 0;
}
extern "C" double nd_twin_condition(const double* A, int n) {
  return nd_twin::condition(std::vector<double>(A, A + n * n), n);
}

// One search from x along d (f, g, H evaluated at x here): the step length, the trial points, and whether the search
// ended at the fixed point of alpha *= rho.
extern "C" int nd_twin_search(int objective, int n, const double* params, const nd_config* cfg, int order, int W,
                              const double* x, const double* d, double* alpha, uint32_t* trials, int32_t* fixed_point) {
  if (n < 1 || n > W) return -1;
  const nd_twin::Objective obj{objective, n, params};
  const nd_twin::Ops o{static_cast<nd_twin::Order>(order), n, order == nd_twin::kDeviceOrder ? W : n};
  std::vector<double> xv(o.L, 0.0), dv(o.L, 0.0), g, H, xt, gt;
  for (int j = 0; j < n; ++j) xv[j] = x[j], dv[j] = d[j];
  const double f = obj.eval(o, xv, g);
  obj.hessian(xv, H);
  const nd_twin::SearchResult r = nd_twin::armijo(obj, o, *cfg, xv, f, g, H, dv, xt, gt);
  *alpha = r.alpha;
  *trials = r.trials;
  *fixed_point = r.fixed_point ? 1 : 0;
  return 0;
}
