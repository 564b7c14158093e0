// ref_harness.cpp — the reference's NelderMead (solver/nelder_mead.h of the reference tree, unmodified) over the Eigen
// stand-in of oracle/eigen_shim with the column arithmetic of overlay/Eigen/Core, behind the C interface of common.h.
// Compiled at test time (or by tests/golden/make_golden_nm.py) into a directory outside the repository; nothing built
// from it is kept in the tree.  The functors restate the device functors' formulas (csrc/objectives.hpp,
// examples/user_objective_l1) with sequential sums and count every call, so that the twin in reference order can match
// them bit for bit, nfev included.  Dynamic dimension: a state built from x alone then has an empty gradient and
// Solver::Minimize rebuilds it (solver.h:210-216), the one evaluation per step the kernel counts.
#include <cstdint>
#include <cstring>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/nelder_mead.h"
#include "common.h"

namespace {
using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;

struct Counter {
  mutable uint32_t nfev = 0;
};

template <class V>
double rosenbrock(const V& x, V* gradient) {
  const int n = static_cast<int>(x.size());
  double f = 0.0;
  for (int i = 0; i + 1 < n; ++i) {
    const double t1 = 1.0 - x[i];
    const double t2 = x[i + 1] - x[i] * x[i];
    const double term = t1 * t1 + (100.0 * t2) * t2;
    f = (i == 0) ? term : f + term;
  }
  if (gradient) {
    *gradient = V::Zero(n);
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
template <class V>
double diag_quadratic(const double* a, const V& x, V* gradient) {
  const int n = static_cast<int>(x.size());
  double f = 0.0;
  if (gradient) *gradient = V::Zero(n);
  for (int i = 0; i < n; ++i) {
    const double term = (a[i] * x[i]) * x[i];
    f = (i == 0) ? term : f + term;
    if (gradient) (*gradient)[i] = (2.0 * a[i]) * x[i];
  }
  return f + a[n];
}

class RosenbrockValue : public FunctionCRTP<RosenbrockValue, double, DifferentiabilityMode::None>, public Counter {
 public:
  const double* params = nullptr;
  ScalarType operator()(const VectorType& x) const {
    ++nfev;
    return rosenbrock<VectorType>(x, nullptr);
  }
};
class RosenbrockFirst : public FunctionCRTP<RosenbrockFirst, double, DifferentiabilityMode::First>, public Counter {
 public:
  const double* params = nullptr;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr) const {
    ++nfev;
    return rosenbrock(x, gradient);
  }
};
class DiagQuadraticValue : public FunctionCRTP<DiagQuadraticValue, double, DifferentiabilityMode::None>, public Counter {
 public:
  const double* params = nullptr;
  ScalarType operator()(const VectorType& x) const {
    ++nfev;
    return diag_quadratic<VectorType>(params, x, nullptr);
  }
};
class DiagQuadraticFirst : public FunctionCRTP<DiagQuadraticFirst, double, DifferentiabilityMode::First>, public Counter {
 public:
  const double* params = nullptr;
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr) const {
    ++nfev;
    return diag_quadratic(params, x, gradient);
  }
};
// f = sum |x_i - c_i| + 0.5 sum (x_i - c_i)^2: d = x_i - c_i, term = |d| + (0.5 d) d
class L1QuadraticValue : public FunctionCRTP<L1QuadraticValue, double, DifferentiabilityMode::None>, public Counter {
 public:
  const double* params = nullptr;
  ScalarType operator()(const VectorType& x) const {
    ++nfev;
    const int n = static_cast<int>(x.size());
    double f = 0.0;
    for (int i = 0; i < n; ++i) {
      const double d = x[i] - params[i];
      const double term = std::fabs(d) + (0.5 * d) * d;
      f = (i == 0) ? term : f + term;
    }
    return f;
  }
};

nm_trajectory* g_sink = nullptr;

// The reference keeps its coefficients as const members with default initialisers and no constructor that takes them
// (nelder_mead.h:58-64).  The cases that need other coefficients write them in place, through a pointer the optimiser
// cannot see through, before the solve starts.
__attribute__((noinline)) void poke(const double& member, double v) {
  double* volatile p = const_cast<double*>(&member);
  *p = v;
}

template <class F>
void solve(F& fn, int n, int64_t B, const nm_stop* st, const nm_config* c, const double* x0, double* x_out, double* f_out,
           double* g_out, nm_progress* prog) {
  using Solver = cppoptlib::solver::NelderMead<F>;
  using State = typename Solver::StateType;
  for (int64_t b = 0; b < B; ++b) {
    typename F::VectorType x(n);
    for (int i = 0; i < n; ++i) x[i] = x0[b * n + i];
    Solver solver;  // the conservative preset with five x_delta strikes (:87-91); the case's stop on top
    auto& stop = solver.stopping_progress;
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
    poke(solver.rho_, c->rho);
    poke(solver.xi_, c->xi);
    poke(solver.gamma_, c->gamma);
    poke(solver.sigma_, c->sigma);
    poke(solver.degenerate_tol_, c->degenerate_tol);
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
    auto [sol, pr] = solver.Minimize(fn, State(x));
    for (int i = 0; i < n; ++i) x_out[b * n + i] = sol.x[i];
    f_out[b] = sol.value;
    for (int i = 0; i < n; ++i) g_out[b * n + i] = (sol.gradient.size() == n) ? sol.gradient[i] : 0.0;
    prog[b].status = static_cast<int32_t>(pr.status);
    prog[b].num_iterations = static_cast<uint32_t>(pr.num_iterations);
    prog[b].nfev = fn.nfev;
    prog[b].sum_k = 0;
    prog[b].x_delta = pr.x_delta;
    prog[b].f_delta = pr.f_delta;
    prog[b].gradient_norm = pr.gradient_norm;
  }
}

template <class F>
int run(const double* params, int n, int64_t B, const nm_stop* st, const nm_config* c, const double* x0, double* x_out,
        double* f_out, double* g_out, nm_progress* prog) {
  F fn;
  fn.params = params;
  solve(fn, n, B, st, c, x0, x_out, f_out, g_out, prog);
  return 0;
}
}  // namespace

// traj (may be null): the per-iteration states of problem 0 as the reference's step callback sees them
extern "C" int nm_ref_solve(int objective, int n, int64_t B, const double* params, const nm_stop* st, const nm_config* cfg,
                            const double* x0, double* x_out, double* f_out, double* g_out, nm_progress* prog,
                            nm_trajectory* traj) {
  if (traj != nullptr) traj->count = 0;
  g_sink = traj;
  int rc = -1;
  const bool first = cfg->mode != 0;
  if (objective == kNmRosenbrock)
    rc = first ? run<RosenbrockFirst>(params, n, B, st, cfg, x0, x_out, f_out, g_out, prog)
               : run<RosenbrockValue>(params, n, B, st, cfg, x0, x_out, f_out, g_out, prog);
  else if (objective == kNmDiagQuadratic)
    rc = first ? run<DiagQuadraticFirst>(params, n, B, st, cfg, x0, x_out, f_out, g_out, prog)
               : run<DiagQuadraticValue>(params, n, B, st, cfg, x0, x_out, f_out, g_out, prog);
  else if (objective == kNmL1Quadratic && !first)
    rc = run<L1QuadraticValue>(params, n, B, st, cfg, x0, x_out, f_out, g_out, prog);
  g_sink = nullptr;
  return rc;
}
