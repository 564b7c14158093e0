// ref_harness.cpp — the reference's GradientDescent and ConjugatedGradientDescent (solver/gradient_descent.h,
// solver/conjugated_gradient_descent.h, linesearch/more_thuente.h and linesearch/armijo.h of the reference tree,
// unmodified) over the Eigen stand-in of oracle/eigen_shim, behind the C interface of common.h.  Compiled at test time
// (or by tests/golden/make_golden_fo.py) into a directory outside the repository; nothing built from it is kept in the
// tree.  The functors restate the device functors' formulas (csrc/objectives.hpp, examples/user_objective_quartic) with
// the reference's sequential sums and count every call, so that the twin in reference order can match them bit for bit,
// nfev included.  Dynamic dimension, as the reference's own test pair uses it (src/test/verify.cc): a state built from x
// alone then has an empty gradient and Solver::Minimize rebuilds it (solver.h:210-216), the one evaluation per step the
// kernel counts.  The reference's Armijo constants (c, rho, alpha_min) are constexpr: the config is not read.
#include <cstdint>
#include <cstring>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/conjugated_gradient_descent.h"
#include "cppoptlib/solver/gradient_descent.h"
#include "common.h"

namespace {
using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;

struct Counter {
  mutable uint32_t nfev = 0;
};

class Rosenbrock : public FunctionCRTP<Rosenbrock, double, DifferentiabilityMode::First>, public Counter {
 public:
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr) const {
    ++nfev;
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
    return f;
  }
};

class DiagQuadratic : public FunctionCRTP<DiagQuadratic, double, DifferentiabilityMode::First>, public Counter {
 public:
  const double* a = nullptr;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr) const {
    ++nfev;
    const int n = static_cast<int>(x.size());
    double f = 0.0;
    if (gradient) *gradient = VectorType::Zero(n);
    for (int i = 0; i < n; ++i) {
      const double term = (a[i] * x[i]) * x[i];
      f = (i == 0) ? term : f + term;
      if (gradient) (*gradient)[i] = (2.0 * a[i]) * x[i];
    }
    return f + a[n];
  }
};

// f = (x_0^2 - 2)^2 in n dimensions: t = x x - 2, f = t t, g_0 = (4 x) t, zero elsewhere
class Quartic : public FunctionCRTP<Quartic, double, DifferentiabilityMode::First>, public Counter {
 public:
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr) const {
    ++nfev;
    const int n = static_cast<int>(x.size());
    const double t = x[0] * x[0] - 2.0;
    if (gradient) {
      *gradient = VectorType::Zero(n);
      (*gradient)[0] = (4.0 * x[0]) * t;
    }
    return t * t;
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

template <class Solver, class F>
void solve(F& fn, int n, int64_t B, const fo_stop* st, const double* x0, double* x_out, double* f_out, double* g_out,
           fo_progress* prog) {
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
    prog[b].sum_k = 0;  // the trial points are not observable from outside the reference's searches on their own
    prog[b].x_delta = pr.x_delta;
    prog[b].f_delta = pr.f_delta;
    prog[b].gradient_norm = pr.gradient_norm;
  }
}

template <class F>
void solve_method(int method, F& fn, int n, int64_t B, const fo_stop* st, const double* x0, double* x_out,
                  double* f_out, double* g_out, fo_progress* prog) {
  if (method == kFoGradientDescent)
    solve<cppoptlib::solver::GradientDescent<F>>(fn, n, B, st, x0, x_out, f_out, g_out, prog);
  else
    solve<cppoptlib::solver::ConjugatedGradientDescent<F>>(fn, n, B, st, x0, x_out, f_out, g_out, prog);
}
}  // namespace

extern "C" int fo_ref_solve(int method, int objective, int n, int64_t B, const double* params, const fo_stop* st,
                            const fo_config* /*cfg*/, const double* x0, double* x_out, double* f_out, double* g_out,
                            fo_progress* prog) {
  if (method != kFoGradientDescent && method != kFoConjugatedGradientDescent) return -1;
  if (objective == kFoRosenbrock) {
    Rosenbrock fn;
    solve_method(method, fn, n, B, st, x0, x_out, f_out, g_out, prog);
  } else if (objective == kFoDiagQuadratic) {
    DiagQuadratic fn;
    fn.a = params;
    solve_method(method, fn, n, B, st, x0, x_out, f_out, g_out, prog);
  } else if (objective == kFoQuartic) {
    Quartic fn;
    solve_method(method, fn, n, B, st, x0, x_out, f_out, g_out, prog);
  } else {
    return -1;
  }
  return 0;
}

// One solve (the first row of x0) with its per-iteration states recorded through the reference's step callback;
// *count = the rows written (at most capacity).
extern "C" int fo_ref_trajectory(int method, int objective, int n, const double* params, const fo_stop* st,
                                 const fo_config* cfg, const double* x0, double* x_out, double* f_out, double* g_out,
                                 fo_progress* prog, int capacity, double* rows, double* xs, int* count) {
  TrajectorySink sink{capacity, rows, xs, 0};
  g_sink = &sink;
  const int rc = fo_ref_solve(method, objective, n, 1, params, st, cfg, x0, x_out, f_out, g_out, prog);
  g_sink = nullptr;
  *count = sink.count;
  return rc;
}
