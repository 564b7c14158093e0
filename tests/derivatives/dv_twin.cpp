// dv_twin.cpp — C interface of the CPU twin (dv_twin.hpp) for tests/dv_lib.py.
#include "dv_twin.hpp"

#include <memory>

namespace {
std::unique_ptr<oracle::Objective> make_objective(int objective, int n, const double* params, int elems) {
  if (objective == kDvRosenbrock) return std::make_unique<oracle::Rosenbrock>();
  if (objective == kDvDiagQuadratic) {
    auto q = std::make_unique<dv_twin::DiagQuadraticHess>();
    q->q.a.assign(params, params + n);
    q->q.c = params[n];
    return q;
  }
  if (objective == kDvQuartic) return std::make_unique<dv_twin::Quartic>();
  if (objective == kDvDense) {
    auto d = std::make_unique<dv_twin::DenseQuartic>();
    d->params = params;
    d->elems = elems;
    return d;
  }
  if (objective == kDvPlanted) {
    auto p = std::make_unique<dv_twin::Planted>();
    p->params = params;
    return p;
  }
  return nullptr;
}
}  // namespace

// width: W x E of the device order (a power of two >= n, at most 1024), elems: E; both ignored in reference order.
// hess / hess_fd null: gradient only.
extern "C" int dv_twin_check(int objective, int n, int64_t B, const double* params, const dv_config* cfg, int order,
                             int width, int elems, const double* x, double* f, double* grad, double* grad_fd,
                             double* hess, double* hess_fd, dv_report* report) {
  if (n < 1 || n > width || width > 1024 || (width & (width - 1)) != 0) return -1;
  if (cfg->gradient_accuracy < 0 || cfg->gradient_accuracy > 3 || cfg->hessian_accuracy < 0 || cfg->hessian_accuracy > 3)
    return -1;
  const auto obj = make_objective(objective, n, params, elems);
  if (!obj) return -1;
  const int64_t nn = static_cast<int64_t>(n) * n;
  for (int64_t b = 0; b < B; ++b)
    dv_twin::check_one(*obj, n, static_cast<dv_twin::Order>(order), width, *cfg, x + b * n, f + b, grad + b * n,
                       grad_fd + b * n, hess ? hess + b * nn : nullptr, hess_fd ? hess_fd + b * nn : nullptr, report + b);
  return 0;
}
