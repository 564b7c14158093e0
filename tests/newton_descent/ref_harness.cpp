// ref_harness.cpp — the reference's NewtonDescent (solver/newton_descent.h and linesearch/armijo.h of the reference
// tree, unmodified) over the Eigen stand-in of oracle/eigen_shim, behind the C interface of common.h.  Compiled at test
// time (or by tests/golden/make_golden_nd.py) into a directory outside the repository; nothing built from it is kept in
// the tree.  The functors restate the device functors' formulas (csrc/objectives.hpp, examples/user_objective_quartic,
// examples/user_objective_dense) with the reference's sequential sums and count every call, so that the twin in
// reference order can match them bit for bit, nfev included.  Dynamic dimension, as the reference's own test pair uses it (src/test/verify.cc): a state built
// from x alone then has an empty gradient and Solver::Minimize rebuilds it (solver.h:210-216), the one evaluation per
// step the kernel counts.  The reference's constants (safe_guard, c, rho) are constexpr: the config is not read.
#include <cstdint>
#include <cstring>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/newton_descent.h"
#include "common.h"

namespace {
using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;

// counts what the reference's solver calls, except Progress::Update's Hessian-only call (progress.h:203-210)
struct Counter {
  mutable uint32_t nfev = 0;
  void count(const void* gradient, const void* hessian) const {
    if (!(gradient == nullptr && hessian != nullptr)) ++nfev;
  }
};

class Rosenbrock : public FunctionCRTP<Rosenbrock, double, DifferentiabilityMode::Second>, public Counter {
 public:
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    count(gradient, hessian);
    const int n = static_cast<int>(x.size());
    double f = 0.0;
    for (int i = 0; i + 1 < n; ++i) {
      const double t1 = 1.0 - x[i];
      const double t2 = x[i + 1] - x[i] * x[i];
      const double term = t1 * t1 + (100.0 * t2) * t2;
      f = (i == 0) ? term : f + term;
    }
    if (gradient) {
      *gradient = VectorType::Zero(n);
      for (int i = 0; i < n; ++i) {
        const bool has_a = (i + 1 < n), has_b = (i > 0);
        double a = 0.0, b = 0.0;
        if (has_a) a = -2.0 * (1.0 - x[i]) + (200.0 * (x[i + 1] - x[i] * x[i])) * (-2.0 * x[i]);
        if (has_b) b = 200.0 * (x[i] - x[i - 1] * x[i - 1]);
        (*gradient)[i] = (has_a && has_b) ? (a + b) : (has_a ? a : b);
      }
    }
    if (hessian) {
      *hessian = MatrixType::Zero(n, n);
      for (int i = 0; i < n; ++i) {
        const bool has_a = (i + 1 < n), has_b = (i > 0);
        const double a = has_a ? ((1200.0 * x[i]) * x[i] - 400.0 * x[i + 1]) + 2.0 : 0.0;
        (*hessian)(i, i) = (has_a && has_b) ? (a + 200.0) : (has_a ? a : (has_b ? 200.0 : 0.0));
        if (has_a) {
          (*hessian)(i, i + 1) = -400.0 * x[i];
          (*hessian)(i + 1, i) = -400.0 * x[i];
        }
      }
    }
    return f;
  }
};

class DiagQuadratic : public FunctionCRTP<DiagQuadratic, double, DifferentiabilityMode::Second>, public Counter {
 public:
  const double* a = nullptr;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    count(gradient, hessian);
    const int n = static_cast<int>(x.size());
    double f = 0.0;
    if (gradient) *gradient = VectorType::Zero(n);
    for (int i = 0; i < n; ++i) {
      const double term = (a[i] * x[i]) * x[i];
      f = (i == 0) ? term : f + term;
      if (gradient) (*gradient)[i] = (2.0 * a[i]) * x[i];
    }
    if (hessian) {
      *hessian = MatrixType::Zero(n, n);
      for (int i = 0; i < n; ++i) (*hessian)(i, i) = 2.0 * a[i];
    }
    return f + a[n];
  }
};

// f = (x_0^2 - 2)^2 in n dimensions: t = x x - 2, f = t t, g_0 = (4 x) t, H_00 = (12 x) x - 8, zero elsewhere
class Quartic : public FunctionCRTP<Quartic, double, DifferentiabilityMode::Second>, public Counter {
 public:
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    count(gradient, hessian);
    const int n = static_cast<int>(x.size());
    const double t = x[0] * x[0] - 2.0;
    if (gradient) {
      *gradient = VectorType::Zero(n);
      (*gradient)[0] = (4.0 * x[0]) * t;
    }
    if (hessian) {
      *hessian = MatrixType::Zero(n, n);
      (*hessian)(0, 0) = (12.0 * x[0]) * x[0] - 8.0;
    }
    return t * t;
  }
};

// the dense quartic of examples/user_objective_dense: f = 0.5 x . (S x) - b . x + (kappa / 4) sum x_i^4 with S column
// major and used as given (H(i, j) = S(i, j), not symmetrised); row i of S x ascending in j, first term a product;
// q_i = x_i x_i, g_i = (sx_i - b_i) + kappa (q_i x_i), H(i, i) = S(i, i) + (3 kappa) q_i;
// f = (0.5 sum x_i sx_i - sum b_i x_i) + (0.25 kappa) sum q_i q_i, each sum ascending
class Dense : public FunctionCRTP<Dense, double, DifferentiabilityMode::Second>, public Counter {
 public:
  const double* params = nullptr;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    count(gradient, hessian);
    const int n = static_cast<int>(x.size());
    const double *S = params, *b = params + n * n, kappa = params[n * n + n];
    double quad = 0.0, lin = 0.0, quart = 0.0;
    if (gradient) *gradient = VectorType::Zero(n);
    for (int i = 0; i < n; ++i) {
      double s = S[i] * x[0];
      for (int j = 1; j < n; ++j) s = s + S[j * n + i] * x[j];
      const double q = x[i] * x[i];
      if (gradient) (*gradient)[i] = (s - b[i]) + kappa * (q * x[i]);
      const double t0 = x[i] * s, t1 = b[i] * x[i], t2 = q * q;
      quad = (i == 0) ? t0 : quad + t0;
      lin = (i == 0) ? t1 : lin + t1;
      quart = (i == 0) ? t2 : quart + t2;
    }
    if (hessian) {
      *hessian = MatrixType::Zero(n, n);
      for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) (*hessian)(i, j) = S[j * n + i];
      for (int i = 0; i < n; ++i) (*hessian)(i, i) = S[i * n + i] + (3.0 * kappa) * (x[i] * x[i]);
    }
    return (0.5 * quad - lin) + (0.25 * kappa) * quart;
  }
};

// where the reference's step callback records the per-iteration states of problem 0 (null = no recording): one row
// (num_iterations, status, value, x_delta, f_delta, gradient_norm) and the iterate per Progress::Update, in order
struct TrajectorySink {
  int capacity;
  double* rows;  // [capacity][6]
  double* xs;    // [capacity][n]
  int count;
};
TrajectorySink* g_sink = nullptr;

template <class F>
void solve(F& fn, int n, int64_t B, const nd_stop* st, double condition_stop, const double* x0, double* x_out,
           double* f_out, double* g_out, nd_progress* prog) {
  using Solver = cppoptlib::solver::NewtonDescent<F>;
  using State = typename Solver::StateType;
  auto stop = cppoptlib::solver::DefaultStoppingSolverProgress<F, State>();
  stop.num_iterations = st->num_iterations;
  stop.x_delta = st->x_delta;
  stop.x_delta_violations = st->x_delta_violations;
  stop.f_delta = st->f_delta;
  stop.f_delta_violations = st->f_delta_violations;
  stop.f_delta_relative = st->f_delta_relative != 0;
  stop.gradient_norm = st->gradient_norm;
  stop.gradient_norm_relative = st->gradient_norm_relative != 0;
  stop.past = st->past;
  stop.past_delta = st->past_delta;
  stop.condition_hessian = condition_stop;
  for (int64_t b = 0; b < B; ++b) {
    typename F::VectorType x(n);
    for (int i = 0; i < n; ++i) x[i] = x0[b * n + i];
    Solver solver(stop);
    if (g_sink != nullptr && b == 0) {
      // solver.h:197 / :222: the callback sees every state after an Update exactly once (plus the start, skipped)
      solver.SetCallback([n](const F&, const State& state, const typename Solver::ProgressType& p) {
        if (p.num_iterations == 0 || g_sink->count >= g_sink->capacity) return;
        double* r = g_sink->rows + 6 * g_sink->count;
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
    prog[b].sum_k = 0;  // the trial points are not observable from outside the reference's search on their own
    prog[b].x_delta = pr.x_delta;
    prog[b].f_delta = pr.f_delta;
    prog[b].gradient_norm = pr.gradient_norm;
  }
}
}  // namespace

extern "C" int nd_ref_solve(int objective, int n, int64_t B, const double* params, const nd_stop* st,
                            double condition_stop, const nd_config* /*cfg*/, const double* x0, double* x_out,
                            double* f_out, double* g_out, nd_progress* prog) {
  if (objective == kNdRosenbrock) {
    Rosenbrock fn;
    solve(fn, n, B, st, condition_stop, x0, x_out, f_out, g_out, prog);
  } else if (objective == kNdDiagQuadratic) {
    DiagQuadratic fn;
    fn.a = params;
    solve(fn, n, B, st, condition_stop, x0, x_out, f_out, g_out, prog);
  } else if (objective == kNdQuartic) {
    Quartic fn;
    solve(fn, n, B, st, condition_stop, x0, x_out, f_out, g_out, prog);
  } else if (objective == kNdDense) {
    Dense fn;
    fn.params = params;
    solve(fn, n, B, st, condition_stop, x0, x_out, f_out, g_out, prog);
  } else {
    return -1;
  }
  return 0;
}

// One solve (the first row of x0) with its per-iteration states recorded through the reference's step callback;
// *count = the rows written (at most capacity).
extern "C" int nd_ref_trajectory(int objective, int n, const double* params, const nd_stop* st, double condition_stop,
                                 const nd_config* cfg, const double* x0, double* x_out, double* f_out, double* g_out,
                                 nd_progress* prog, int capacity, double* rows, double* xs, int* count) {
  TrajectorySink sink{capacity, rows, xs, 0};
  g_sink = &sink;
  const int rc = nd_ref_solve(objective, n, 1, params, st, condition_stop, cfg, x0, x_out, f_out, g_out, prog);
  g_sink = nullptr;
  *count = sink.count;
  return rc;
}
