// at_twin.cpp — the C interface of the ask/tell twin (at_twin.hpp) for tests/at_lib.py: create / x / tell / results /
// drive / destroy, shaped like the library's mi355_lbfgs_ask_tell_* entry points.  order: 0 sequential (the reference's),
// 1 butterfly over `width` (the device's, width = lanes x coordinates per lane).
#include "at_twin.hpp"

extern "C" {

void* at_create(int n, int m, const at_stop* stop, int order, int width, int64_t B, const double* x0) {
  if (n < 1 || m < 1 || !stop || B < 0 || (B > 0 && !x0) || width < n || width > 1024 || (width & (width - 1))) return nullptr;
  return new at_twin::Batch(n, m, *stop, order, width, B, x0);
}
double* at_x(void* h) { return static_cast<at_twin::Batch*>(h)->x_eval.data(); }
int64_t at_tell(void* h, const double* f, const double* g) { return static_cast<at_twin::Batch*>(h)->tell(f, g); }
void at_results(void* h, double* x, double* f, double* g, at_progress* progress) {
  static_cast<at_twin::Batch*>(h)->results(x, f, g, progress);
}
// The whole loop in one call, for large batches: the callback is the oracle's functor (0 Rosenbrock, 1 DiagQuadratic with
// params a[n], c) in the batch's own summation order.  Returns the number of rounds, -1 for an unknown objective or when
// max_rounds did not finish the batch.
int64_t at_drive(void* h, int objective, const double* params, int64_t max_rounds) {
  at_twin::Batch& batch = *static_cast<at_twin::Batch*>(h);
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
void at_destroy(void* h) { delete static_cast<at_twin::Batch*>(h); }

}  // extern "C"
