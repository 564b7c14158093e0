// ref_harness.cpp — the reference's TrustRegionNewton (solver/trust_region_newton.h of the reference tree, unmodified)
// over the Eigen stand-in of oracle/eigen_shim, behind the C interface of common.h.  Compiled at test time (or by
// tests/golden/make_golden_tr.py) into a directory outside the repository; nothing built from it is kept in the tree.
// The functors restate the device functors' formulas (csrc/objectives.hpp, examples/user_objective_quartic,
// examples/user_objective_dense), with the reference's sequential sums, so that the twin in reference order can match
// them bit for bit.
#include <cstdint>
#include <cstring>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/trust_region_newton.h"
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

template <int N>
class Rosenbrock : public FunctionCRTP<Rosenbrock<N>, double, DifferentiabilityMode::Second, N>, public Counter {
 public:
  using typename FunctionCRTP<Rosenbrock<N>, double, DifferentiabilityMode::Second, N>::ScalarType;
  using typename FunctionCRTP<Rosenbrock<N>, double, DifferentiabilityMode::Second, N>::VectorType;
  using typename FunctionCRTP<Rosenbrock<N>, double, DifferentiabilityMode::Second, N>::MatrixType;
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
      *gradient = VectorType::Zero();
      for (int i = 0; i < n; ++i) {
        const bool has_a = (i + 1 < n), has_b = (i > 0);
        double a = 0.0, b = 0.0;
        if (has_a) a = -2.0 * (1.0 - x[i]) + (200.0 * (x[i + 1] - x[i] * x[i])) * (-2.0 * x[i]);
        if (has_b) b = 200.0 * (x[i] - x[i - 1] * x[i - 1]);
        (*gradient)[i] = (has_a && has_b) ? (a + b) : (has_a ? a : b);
      }
    }
    if (hessian) {
      *hessian = MatrixType::Zero();
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

template <int N>
class DiagQuadratic : public FunctionCRTP<DiagQuadratic<N>, double, DifferentiabilityMode::Second, N>, public Counter {
 public:
  using typename FunctionCRTP<DiagQuadratic<N>, double, DifferentiabilityMode::Second, N>::ScalarType;
  using typename FunctionCRTP<DiagQuadratic<N>, double, DifferentiabilityMode::Second, N>::VectorType;
  using typename FunctionCRTP<DiagQuadratic<N>, double, DifferentiabilityMode::Second, N>::MatrixType;
 public:
  const double* a = nullptr;
  double c = 0.0;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    count(gradient, hessian);
    const int n = static_cast<int>(x.size());
    double f = 0.0;
    if (gradient) *gradient = VectorType::Zero();
    for (int i = 0; i < n; ++i) {
      const double term = (a[i] * x[i]) * x[i];
      f = (i == 0) ? term : f + term;
      if (gradient) (*gradient)[i] = (2.0 * a[i]) * x[i];
    }
    if (hessian) {
      *hessian = MatrixType::Zero();
      for (int i = 0; i < n; ++i) (*hessian)(i, i) = 2.0 * a[i];
    }
    return f + c;
  }
};

// f = (x^2 - 2)^2 (trust_region_newton_test.cc's double well): t = x x - 2, f = t t, g = (4 x) t, H = (12 x) x - 8
class Quartic : public FunctionCRTP<Quartic, double, DifferentiabilityMode::Second, 1>, public Counter {
 public:
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    count(gradient, hessian);
    const double t = x[0] * x[0] - 2.0;
    if (gradient) {
      *gradient = VectorType::Zero();
      (*gradient)[0] = (4.0 * x[0]) * t;
    }
    if (hessian) {
      *hessian = MatrixType::Zero();
      (*hessian)(0, 0) = (12.0 * x[0]) * x[0] - 8.0;
    }
    return t * t;
  }
};

// the dense quartic of examples/user_objective_dense: f = 0.5 x . (S x) - b . x + (kappa / 4) sum x_i^4 with S column
// major and used as given (H(i, j) = S(i, j), not symmetrised); row i of S x ascending in j, first term a product;
// q_i = x_i x_i, g_i = (sx_i - b_i) + kappa (q_i x_i), H(i, i) = S(i, i) + (3 kappa) q_i;
// f = (0.5 sum x_i sx_i - sum b_i x_i) + (0.25 kappa) sum q_i q_i, each sum ascending
template <int N>
class Dense : public FunctionCRTP<Dense<N>, double, DifferentiabilityMode::Second, N>, public Counter {
 public:
  using typename FunctionCRTP<Dense<N>, double, DifferentiabilityMode::Second, N>::ScalarType;
  using typename FunctionCRTP<Dense<N>, double, DifferentiabilityMode::Second, N>::VectorType;
  using typename FunctionCRTP<Dense<N>, double, DifferentiabilityMode::Second, N>::MatrixType;
 public:
  const double* params = nullptr;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr, MatrixType* hessian = nullptr) const {
    count(gradient, hessian);
    const int n = static_cast<int>(x.size());
    const double *S = params, *b = params + n * n, kappa = params[n * n + n];
    double quad = 0.0, lin = 0.0, quart = 0.0;
    if (gradient) *gradient = VectorType::Zero();
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
      *hessian = MatrixType::Zero();
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
void solve(F& fn, int n, int64_t B, const tr_stop* st, double condition_stop, const tr_config* c, const double* x0,
           double* x_out, double* f_out, double* g_out, tr_progress* prog) {
  using Solver = cppoptlib::solver::TrustRegionNewton<F>;
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
  typename Solver::Config cfg;
  cfg.initial_radius = c->initial_radius;
  cfg.max_radius = c->max_radius;
  cfg.acceptance_threshold = c->acceptance_threshold;
  cfg.shrink_factor = c->shrink_factor;
  cfg.expand_factor = c->expand_factor;
  cfg.rho_low = c->rho_low;
  cfg.rho_high = c->rho_high;
  cfg.cg_forcing_coefficient = c->cg_forcing_coefficient;
  cfg.cg_max_iterations_floor = c->cg_max_iterations_floor;
  cfg.min_radius = c->min_radius;
  cfg.rejection_retry_limit = c->rejection_retry_limit;
  for (int64_t b = 0; b < B; ++b) {
    typename F::VectorType x;
    for (int i = 0; i < n; ++i) x[i] = x0[b * n + i];
    Solver solver(stop, cfg);
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
    prog[b].sum_k = 0;  // the CG iterations are not observable from outside the reference's solver
    prog[b].x_delta = pr.x_delta;
    prog[b].f_delta = pr.f_delta;
    prog[b].gradient_norm = pr.gradient_norm;
  }
}

// The reference's TrustRegionNewton needs a compile-time dimension: InitializeSolver leaves dim_ at 0
// (trust_region_newton.h:184-187), so a dynamic-size problem gets zero-length CG vectors; a fixed-size one gets its full
// length from VectorType::Zero().  The harness therefore instantiates the dimensions the tests use.
template <int N>
int solve_n(int objective, int64_t B, const double* params, const tr_stop* st, double condition_stop, const tr_config* cfg,
            const double* x0, double* x_out, double* f_out, double* g_out, tr_progress* prog) {
  if (objective == kTrRosenbrock) {
    Rosenbrock<N> fn;
    solve(fn, N, B, st, condition_stop, cfg, x0, x_out, f_out, g_out, prog);
  } else if (objective == kTrDiagQuadratic) {
    DiagQuadratic<N> fn;
    fn.a = params;
    fn.c = params[N];
    solve(fn, N, B, st, condition_stop, cfg, x0, x_out, f_out, g_out, prog);
  } else if (objective == kTrDense) {
    Dense<N> fn;
    fn.params = params;
    solve(fn, N, B, st, condition_stop, cfg, x0, x_out, f_out, g_out, prog);
  } else if (objective == kTrQuartic && N == 1) {
    Quartic fn;
    solve(fn, 1, B, st, condition_stop, cfg, x0, x_out, f_out, g_out, prog);
  } else {
    return -1;
  }
  return 0;
}
}  // namespace

extern "C" int tr_ref_solve(int objective, int n, int64_t B, const double* params, const tr_stop* st,
                            double condition_stop, const tr_config* cfg, const double* x0, double* x_out, double* f_out,
                            double* g_out, tr_progress* prog) {
  switch (n) {
#define TR_N(N) case N: return solve_n<N>(objective, B, params, st, condition_stop, cfg, x0, x_out, f_out, g_out, prog);
    TR_N(1) TR_N(2) TR_N(3) TR_N(4) TR_N(5) TR_N(6) TR_N(7) TR_N(8) TR_N(9) TR_N(12) TR_N(16) TR_N(17) TR_N(32)
    TR_N(33) TR_N(63) TR_N(64)
#undef TR_N
  }
  return -1;
}

// One solve (the first row of x0) with its per-iteration states recorded through the reference's step callback;
// *count = the rows written (at most capacity).
extern "C" int tr_ref_trajectory(int objective, int n, const double* params, const tr_stop* st, double condition_stop,
                                 const tr_config* cfg, const double* x0, double* x_out, double* f_out, double* g_out,
                                 tr_progress* prog, int capacity, double* rows, double* xs, int* count) {
  TrajectorySink sink{capacity, rows, xs, 0};
  g_sink = &sink;
  const int rc = tr_ref_solve(objective, n, 1, params, st, condition_stop, cfg, x0, x_out, f_out, g_out, prog);
  g_sink = nullptr;
  *count = sink.count;
  return rc;
}
