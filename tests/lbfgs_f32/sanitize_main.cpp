// sanitize_main.cpp — a stand-alone run of the float twin for the Makefile's `sanitize` target (address + undefined
// behaviour sanitizers, CPU only): three cases, both summation orders, printed so the run cannot be optimised away.
#include <cstdio>

#include "f32_twin.hpp"

namespace {
int run(int objective, int n, int m, int width, int past) {
  l32_stop st{10000, 1e-9, 1, 0.0, 1, 0, 1e-5, 1, past, 1e-6};
  std::vector<double> params(n + 1);
  for (int j = 0; j < n; ++j) params[j] = 0.5 + 49.5 * j / n;
  params[n] = 0.25;
  std::vector<float> x0(n), x(n), g(n);
  for (int j = 0; j < n; ++j) x0[j] = (j % 2) ? 1.0f : -1.2f;
  int bad = 0;
  for (int order = 0; order < 2; ++order) {
    float f = 0;
    l32_progress p{};
    std::vector<double> rows(64 * kL32RowWidth);
    std::vector<float> xs(64 * n);
    f32_twin::Trajectory t{64, rows.data(), xs.data(), 0};
    f32_twin::solve_one(objective, params.data(), n, m, static_cast<f32_twin::Order>(order), width, st, x0.data(), x.data(),
                        &f, g.data(), &p, &t);
    std::printf("objective %d n %d m %d order %d: status %d iterations %u nfev %u f %.9g\n", objective, n, m, order,
                p.status, p.num_iterations, p.nfev, static_cast<double>(f));
    if (p.status <= 0 || !(f == f)) bad = 1;
  }
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  bad |= run(kL32Rosenbrock, 2, 6, 8, 3);
  bad |= run(kL32Rosenbrock, 13, 3, 16, 0);
  bad |= run(kL32DiagQuadratic, 65, 10, 128, 3);
  return bad;
}
