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
