// sanitize_main.cpp — a stand-alone run of the ask/tell twin for the Makefile's `sanitize` target (address + undefined
// behaviour sanitizers, CPU only): three cases in both summation orders, the objective evaluated by the oracle's functors
// between the steps, printed so the run cannot be optimised away.
#include <cstdio>
#include <memory>

#include "at_twin.hpp"

namespace {
int run(int objective, int n, int m, int width, int past, double poison) {
  const at_stop st{200, 1e-9, 1, 0.0, 1, 0, 1e-5, 1, past, 1e-6};
  std::unique_ptr<oracle::Objective> fun;
  if (objective == 0) {
    fun.reset(new oracle::Rosenbrock);
  } else {
    auto* q = new oracle::DiagQuadratic;
    for (int j = 0; j < n; ++j) q->a.push_back(0.5 + 49.5 * j / n);
    q->c = 0.25;
    fun.reset(q);
  }
  const int B = 3;
  std::vector<double> x0(static_cast<size_t>(B) * n);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < n; ++j) x0[static_cast<size_t>(b) * n + j] = ((j % 2) ? 1.0 : -1.2) + 0.05 * b;
  int bad = 0;
  for (int order = 0; order < 2; ++order) {
    at_twin::Batch batch(n, m, st, order, width, B, x0.data());
    std::vector<double> f(B), g(static_cast<size_t>(B) * n);
    int64_t active = B;
    int rounds = 0;
    while (active > 0 && rounds < 100000) {
      for (int b = 0; b < B; ++b) {
        if (batch.problems[b].phase == at_twin::kFinished) {  // rows of finished problems are never read
          f[b] = poison;
          for (int j = 0; j < n; ++j) g[static_cast<size_t>(b) * n + j] = poison;
          continue;
        }
        f[b] = fun->eval(batch.x_eval.data() + static_cast<size_t>(b) * n, g.data() + static_cast<size_t>(b) * n, n, batch.red);
      }
      active = batch.tell(f.data(), g.data());
      ++rounds;
    }
    std::vector<at_progress> p(B);
    std::vector<double> fo(B);
    batch.results(nullptr, fo.data(), nullptr, p.data());
    for (int b = 0; b < B; ++b) {
      std::printf("objective %d n %d m %d order %d problem %d: rounds %d status %d iterations %u nfev %u f %.17g\n", objective, n,
                  m, order, b, rounds, p[b].status, p[b].num_iterations, p[b].nfev, fo[b]);
      if (p[b].status <= 0 || !(fo[b] == fo[b])) bad = 1;
    }
  }
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  bad |= run(0, 2, 6, 8, 3, std::numeric_limits<double>::quiet_NaN());
  bad |= run(0, 13, 3, 16, 0, 1e300);
  bad |= run(1, 65, 10, 128, 3, std::numeric_limits<double>::quiet_NaN());
  return bad;
}
