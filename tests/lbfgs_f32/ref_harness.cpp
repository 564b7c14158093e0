// ref_harness.cpp — the reference's Lbfgs<F, m, MoreThuente> (solver/lbfgs.h, linesearch/more_thuente.h, solver/solver.h
// and solver/progress.h of the reference tree, unmodified) instantiated on FLOAT functors over the Eigen stand-in of
// oracle/eigen_shim, behind the C interface of common.h, for m in {1, 3, 6, 10}.  Compiled at test time (or by
// tests/golden/make_golden_f32.py) into a directory outside the repository; nothing built from it is kept in the tree.
// The functors restate the device functors' formulas (csrc/objectives_f32.hpp) with sequential sums and count every
// call, so that the twin in reference order can match them bit for bit, nfev included.
#include <cstdint>
#include <vector>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/lbfgs.h"
#include "common.h"

namespace {
using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;

struct Counter {
  mutable uint32_t nfev = 0;
};

class Rosenbrock : public FunctionCRTP<Rosenbrock, float, DifferentiabilityMode::First>, public Counter {
 public:
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr) const {
    ++nfev;
    const int n = static_cast<int>(x.size());
    float f = 0.0f;
    for (int i = 0; i + 1 < n; ++i) {
      const float t1 = 1.0f - x[i];
      const float t2 = x[i + 1] - x[i] * x[i];
      const float term = t1 * t1 + (100.0f * t2) * t2;
      f = (i == 0) ? term : f + term;
    }
    if (gradient) {
      *gradient = VectorType::Zero(n);
      for (int i = 0; i < n; ++i) {
        const bool has_a = (i + 1 < n), has_b = (i > 0);
        float a = 0.0f, b = 0.0f;
        if (has_a) a = -2.0f * (1.0f - x[i]) + (200.0f * (x[i + 1] - x[i] * x[i])) * (-2.0f * x[i]);
        if (has_b) b = 200.0f * (x[i] - x[i - 1] * x[i - 1]);
        (*gradient)[i] = (has_a && has_b) ? (a + b) : (has_a ? a : b);
      }
    }
    return f;
  }
};

class DiagQuadratic : public FunctionCRTP<DiagQuadratic, float, DifferentiabilityMode::First>, public Counter {
 public:
  std::vector<float> a;  // a[0 .. n), c
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr) const {
    ++nfev;
    const int n = static_cast<int>(x.size());
    float f = 0.0f;
    if (gradient) *gradient = VectorType::Zero(n);
    for (int i = 0; i < n; ++i) {
      const float term = (a[i] * x[i]) * x[i];
      f = (i == 0) ? term : f + term;
      if (gradient) (*gradient)[i] = (2.0f * a[i]) * x[i];
    }
    return f + a[n];
  }
};

struct TrajectorySink {
  int capacity;
  double* rows;
  float* xs;
  int count;
};
TrajectorySink* g_sink = nullptr;

template <int M, class F>
void solve(F& fn, int n, int64_t B, const l32_stop* st, const float* x0, float* x_out, float* f_out, float* g_out,
           l32_progress* prog) {
  using Solver = cppoptlib::solver::Lbfgs<F, M>;
  using State = typename Solver::StateType;
  auto stop = cppoptlib::solver::DefaultStoppingSolverProgress<F, State>();
  stop.num_iterations = st->num_iterations;
  stop.x_delta = static_cast<float>(st->x_delta);
  stop.x_delta_violations = st->x_delta_violations;
  stop.f_delta = static_cast<float>(st->f_delta);
  stop.f_delta_violations = st->f_delta_violations;
  stop.f_delta_relative = st->f_delta_relative != 0;
  stop.gradient_norm = static_cast<float>(st->gradient_norm);
  stop.gradient_norm_relative = st->gradient_norm_relative != 0;
  stop.past = st->past;
  stop.past_delta = static_cast<float>(st->past_delta);
  for (int64_t b = 0; b < B; ++b) {
    typename F::VectorType x(n);
    for (int i = 0; i < n; ++i) x[i] = x0[b * n + i];
    Solver solver(stop);
    if (g_sink != nullptr && b == 0) {
      solver.SetCallback([n](const F&, const State& state, const typename Solver::ProgressType& p) {
        if (p.num_iterations == 0 || g_sink->count >= g_sink->capacity) return;
        double* r = g_sink->rows + kL32RowWidth * g_sink->count;
        r[0] = static_cast<double>(p.num_iterations);
        r[1] = static_cast<double>(static_cast<int>(p.status));
        r[2] = state.value;
        r[3] = p.x_delta;
        r[4] = p.f_delta;
        r[5] = p.gradient_norm;
        for (int i = 0; i < n; ++i) g_sink->xs[g_sink->count * n + i] = state.x[i];
        ++g_sink->count;
      });
    }
    fn.nfev = 0;
    auto [sol, pr] = solver.Minimize(fn, cppoptlib::function::FunctionState(x));
    for (int i = 0; i < n; ++i) x_out[b * n + i] = sol.x[i];
    f_out[b] = sol.value;
    for (int i = 0; i < n; ++i) g_out[b * n + i] = sol.gradient[i];
    prog[b].status = static_cast<int32_t>(pr.status);
    prog[b].num_iterations = static_cast<uint32_t>(pr.num_iterations);
    prog[b].nfev = fn.nfev;
    prog[b].sum_k = 0;  // not observable from outside the reference's step
    prog[b].x_delta = pr.x_delta;
    prog[b].f_delta = pr.f_delta;
    prog[b].gradient_norm = pr.gradient_norm;
  }
}

template <class F>
int solve_m(int m, F& fn, int n, int64_t B, const l32_stop* st, const float* x0, float* x_out, float* f_out, float* g_out,
            l32_progress* prog) {
  switch (m) {
    case 1: solve<1>(fn, n, B, st, x0, x_out, f_out, g_out, prog); return 0;
    case 3: solve<3>(fn, n, B, st, x0, x_out, f_out, g_out, prog); return 0;
    case 6: solve<6>(fn, n, B, st, x0, x_out, f_out, g_out, prog); return 0;
    case 10: solve<10>(fn, n, B, st, x0, x_out, f_out, g_out, prog); return 0;
  }
  return -1;
}
}  // namespace

extern "C" int l32_ref_solve(int objective, int n, int m, int64_t B, const double* params, const l32_stop* st,
                             const float* x0, float* x_out, float* f_out, float* g_out, l32_progress* prog) {
  if (objective == kL32Rosenbrock) {
    Rosenbrock fn;
    return solve_m(m, fn, n, B, st, x0, x_out, f_out, g_out, prog);
  }
  if (objective == kL32DiagQuadratic) {
    DiagQuadratic fn;
    fn.a.resize(n + 1);
    for (int i = 0; i <= n; ++i) fn.a[i] = static_cast<float>(params[i]);
    return solve_m(m, fn, n, B, st, x0, x_out, f_out, g_out, prog);
  }
  return -1;
}

extern "C" int l32_ref_trajectory(int objective, int n, int m, const double* params, const l32_stop* st, const float* x0,
                                  float* x_out, float* f_out, float* g_out, l32_progress* prog, int capacity,
                                  double* rows, float* xs, int* count) {
  TrajectorySink sink{capacity, rows, xs, 0};
  g_sink = &sink;
  const int rc = l32_ref_solve(objective, n, m, 1, params, st, x0, x_out, f_out, g_out, prog);
  g_sink = nullptr;
  *count = sink.count;
  return rc;
}
