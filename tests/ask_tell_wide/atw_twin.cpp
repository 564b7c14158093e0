// atw_twin.cpp — the C interface of the ask/tell twin above n = 256 (atw_twin.hpp) for tests/atw_lib.py: create / x /
// tell / results / drive / destroy, shaped like the library's mi355_lbfgs_ask_tell_wide_* entry points.  width: the lanes
// of the strided order (256, or 1024 for n >= 32768).
#include "atw_twin.hpp"

extern "C" {

void* atw_create(int n, int m, const at_stop* stop, int width, int64_t B, const double* x0) {
  if (n < 1 || m < 1 || !stop || B < 0 || (B > 0 && !x0) || width < 1 || width > 1024 || (width & (width - 1))) return nullptr;
  return new atw_twin::Batch(n, m, *stop, width, B, x0);
}
double* atw_x(void* h) { return static_cast<atw_twin::Batch*>(h)->x_eval.data(); }
int64_t atw_tell(void* h, const double* f, const double* g) { return static_cast<atw_twin::Batch*>(h)->tell(f, g); }
void atw_results(void* h, double* x, double* f, double* g, at_progress* progress) {
  static_cast<atw_twin::Batch*>(h)->results(x, f, g, progress);
}
// The whole loop in one call: the callback is the oracle's functor (0 Rosenbrock, 1 DiagQuadratic with params a[n], c)
// in the batch's own summation order.  Returns the number of rounds, -1 for an unknown objective or when max_rounds
// did not finish the batch.
int64_t atw_drive(void* h, int objective, const double* params, int64_t max_rounds) {
  atw_twin::Batch& batch = *static_cast<atw_twin::Batch*>(h);
  oracle::Rosenbrock rosenbrock;
  oracle::DiagQuadratic quadratic;
  const oracle::Objective* fun = &rosenbrock;
  if (objective == 1) {
    if (!params) return -1;
    quadratic.a.assign(params, params + batch.n);
    quadratic.c = params[batch.n];
    fun = &quadratic;
  } else if (objective != 0) {
    return -1;
  }
  const size_t B = batch.problems.size();
  std::vector<double> f(B), g(B * batch.n);
  int64_t rounds = 0, active = static_cast<int64_t>(B);
  while (active > 0) {
    if (rounds >= max_rounds) return -1;
    for (size_t b = 0; b < B; ++b)
      f[b] = fun->eval(batch.x_eval.data() + b * batch.n, g.data() + b * batch.n, batch.n, batch.red);
    active = batch.tell(f.data(), g.data());
    ++rounds;
  }
  return rounds;
}
// One evaluation of the oracle's functor (0 Rosenbrock, 1 DiagQuadratic with params a[n], c) in the STRIDED order of
// `width` lanes: what oracle.minimize_batch(reduction="strided") evaluates with.  (oracle_eval of oracle/oracle_capi.cpp
// knows the sequential and the butterfly order only: asked for "strided" it runs the butterfly over the first `width`
// terms.)  Returns f, writes g[n]; NaN for an unknown objective.
double atw_eval(int objective, const double* params, int n, int width, const double* x, double* g) {
  oracle::Reducer red;
  red.kind = oracle::Reduction::Strided;
  red.width = width;
  if (objective == 0) return oracle::Rosenbrock().eval(x, g, n, red);
  if (objective == 1 && params) {
    oracle::DiagQuadratic quadratic;
    quadratic.a.assign(params, params + n);
    quadratic.c = params[n];
    return quadratic.eval(x, g, n, red);
  }
  return std::numeric_limits<double>::quiet_NaN();
}
void atw_destroy(void* h) { delete static_cast<atw_twin::Batch*>(h); }

}  // extern "C"
