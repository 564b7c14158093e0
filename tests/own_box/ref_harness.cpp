// Reference harness of the per-problem-bounds tests: the reference's own Lbfgsb<F, 7> (solver/lbfgsb.h over the Eigen
// stand-in) on the chained Rosenbrock function, ONE SetBounds box per row.  The reference binary the other tests use
// holds no history size 7 on this function; this file is compiled by hand into a directory outside the tree
// (tests/golden/make_golden_own_box.py) and its results are recorded under tests/golden/.
#include <cstdint>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/lbfgsb.h"

namespace {
using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;

// chained Rosenbrock-N in the operation order of the project's oracle (oracle/lbfgs_oracle.hpp)
class RosenbrockN : public FunctionCRTP<RosenbrockN, double, DifferentiabilityMode::First> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* gradient = nullptr) const {
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
}  // namespace

// the stopping fields in the order of tests/oracle_lib.py's Stop
struct own_box_stop {
  uint64_t num_iterations;
  double x_delta;
  int32_t x_delta_violations;
  double f_delta;
  int32_t f_delta_violations;
  int32_t f_delta_relative;
  double gradient_norm;
  int32_t gradient_norm_relative;
  int32_t past;
  double past_delta;
};

extern "C" int own_box_ref_rosenbrock_m7(int n, int64_t B, const own_box_stop* st, const double* lower, const double* upper,
                                         const double* x0, double* x_out, double* f_out, int32_t* status_out,
                                         uint32_t* iterations_out) {
  using Solver = cppoptlib::solver::Lbfgsb<RosenbrockN, 7>;
  using State = Solver::StateType;
  auto stop = cppoptlib::solver::DefaultStoppingSolverProgress<RosenbrockN, State>();
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
  RosenbrockN fn;
  for (int64_t b = 0; b < B; ++b) {
    RosenbrockN::VectorType x(n), lo(n), hi(n);
    for (int i = 0; i < n; ++i) {
      x[i] = x0[b * n + i];
      lo[i] = lower[b * n + i];
      hi[i] = upper[b * n + i];
    }
    Solver solver(stop);
    solver.SetBounds(lo, hi);
    auto [solution, progress] = solver.Minimize(fn, cppoptlib::function::FunctionState(x));
    for (int i = 0; i < n; ++i) x_out[b * n + i] = solution.x[i];
    f_out[b] = solution.value;
    status_out[b] = static_cast<int32_t>(progress.status);
    iterations_out[b] = static_cast<uint32_t>(progress.num_iterations);
  }
  return 0;
}
