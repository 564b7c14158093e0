// The NelderMead scenarios of the reference's src/test/verify.cc (SOLVER_SETUP(NelderMead, RosenbrockValue): Far from
// (15, 8), Near from (-1, 2), default-constructed solver, |f(x*)| < 1e-4) restated over the drop-in header
// include/cppoptlib/solver/nelder_mead.h (device solves).  The functors are ours: each states its device twin in one line.
// `nm_header_test --preset` checks the constructors only and touches no device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/nelder_mead.h"
#include "mini_test.h"

using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;
using cppoptlib::function::FunctionState;
using cppoptlib::solver::NelderMead;
namespace twin = cppoptlib::mi355::twin;

// verify.cc:36-50: a value and nothing else
class RosenbrockValue : public FunctionCRTP<RosenbrockValue, double, DifferentiabilityMode::None> {
 public:
  ScalarType operator()(const VectorType& x) const {
    const double t1 = (1 - x[0]);
    const double t2 = (x[1] - x[0] * x[0]);
    return t1 * t1 + 100 * t2 * t2;
  }
  auto DeviceTwin() const { return twin::Rosenbrock(); }
};

class RosenbrockGradient : public FunctionCRTP<RosenbrockGradient, double, DifferentiabilityMode::First> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* grad = nullptr) const {
    const double t1 = (1 - x[0]);
    const double t2 = (x[1] - x[0] * x[0]);
    if (grad) {
      *grad = VectorType(2);
      (*grad)[0] = -2 * t1 + 200 * t2 * (-2 * x[0]);
      (*grad)[1] = 200 * t2;
    }
    return t1 * t1 + 100 * t2 * t2;
  }
  auto DeviceTwin() const { return twin::Rosenbrock(); }
};

template <class F>
typename F::VectorType vec(double a, double b) {
  typename F::VectorType x(2);
  x[0] = a;
  x[1] = b;
  return x;
}

int main(int argc, char** argv) {
  {  // nelder_mead.h:87-91: the conservative preset with five x_delta strikes; a given progress is taken as it is
    NelderMead<RosenbrockValue> solver;
    const auto conservative =
        cppoptlib::solver::ConservativeStoppingSolverProgress<RosenbrockValue, NelderMead<RosenbrockValue>::StateType>();
    EXPECT_EQ(solver.stopping_progress.x_delta_violations, 5);
    EXPECT_EQ(solver.stopping_progress.past, conservative.past);
    EXPECT_EQ(solver.stopping_progress.past, 5);
    EXPECT_EQ(solver.stopping_progress.past_delta, conservative.past_delta);
    EXPECT_EQ(solver.stopping_progress.gradient_norm, conservative.gradient_norm);
    EXPECT_EQ(solver.stopping_progress.x_delta, conservative.x_delta);
    NelderMead<RosenbrockValue> given(conservative);
    EXPECT_EQ(given.stopping_progress.x_delta_violations, 1);
    EXPECT_EQ(solver.rho_, 1.0);
    EXPECT_EQ(solver.xi_, 20.0);
    EXPECT_EQ(solver.gamma_, 0.1);
    EXPECT_EQ(solver.sigma_, 0.5);
    EXPECT_EQ(solver.degenerate_tol_, 1e-8);
  }
  if (argc > 1 && std::strcmp(argv[1], "--preset") == 0) TEST_MAIN_END();
  const double starts[2][2] = {{15.0, 8.0}, {-1.0, 2.0}};  // Far, Near
  for (const auto& s0 : starts) {
    RosenbrockValue f;
    NelderMead<RosenbrockValue> solver;
    auto [solution, state] = solver.Minimize(f, FunctionState(vec<RosenbrockValue>(s0[0], s0[1])));
    EXPECT_NEAR(0.0, f(solution.x), 1e-4);
    EXPECT_TRUE(state.status != cppoptlib::solver::Status::IterationLimit);
    EXPECT_EQ(state.gradient_norm, 0.0);
  }
  {  // the callback, replayed from the device trace: the start, then one state per iteration, values never rising
    RosenbrockValue f;
    NelderMead<RosenbrockValue> solver;
    size_t calls = 0, last_iteration = 0;
    double last_value = 0.0;
    bool monotone = true, in_order = true;
    solver.SetCallback([&](const RosenbrockValue&, const auto& state, const auto& prog) {
      if (calls > 0 && state.value > last_value) monotone = false;
      if (calls > 0 && prog.num_iterations != last_iteration + 1) in_order = false;
      last_value = state.value;
      last_iteration = prog.num_iterations;
      ++calls;
    });
    auto [solution, state] = solver.Minimize(f, FunctionState(vec<RosenbrockValue>(-1.0, 2.0)));
    EXPECT_EQ(calls, static_cast<size_t>(state.num_iterations) + 1);
    EXPECT_TRUE(monotone);
    EXPECT_TRUE(in_order);
    EXPECT_EQ(last_value, solution.value);
  }
  {  // a First-mode function: the same vertices, value and gradient at the returned one
    RosenbrockGradient f;
    NelderMead<RosenbrockGradient> solver;
    solver.stopping_progress.gradient_norm = 0;   // (the gradient test off: the walk is the value-mode one)
    auto [solution, state] = solver.Minimize(f, FunctionState(vec<RosenbrockGradient>(-1.0, 2.0)));
    RosenbrockValue fv;
    NelderMead<RosenbrockValue> value_solver;
    auto [vs, vp] = value_solver.Minimize(fv, FunctionState(vec<RosenbrockValue>(-1.0, 2.0)));
    EXPECT_EQ(solution.x[0], vs.x[0]);
    EXPECT_EQ(solution.x[1], vs.x[1]);
    EXPECT_EQ(solution.value, vs.value);
    EXPECT_EQ(state.num_iterations, vp.num_iterations);
    EXPECT_TRUE(state.gradient_norm > 0.0);
  }
  {  // the batched entry point
    RosenbrockValue f;
    NelderMead<RosenbrockValue> solver;
    std::vector<NelderMead<RosenbrockValue>::StateType> batch;
    for (int b = 0; b < 16; ++b) batch.emplace_back(vec<RosenbrockValue>(-1.2 + 0.1 * b, 1.0 - 0.05 * b));
    auto out = solver.MinimizeBatch(f, batch);
    EXPECT_EQ(out.size(), size_t(16));
    for (size_t b = 0; b < out.size(); ++b) {   // each problem of the batch is the single solve from its start
      auto& [s, p] = out[b];
      auto [one, one_p] = solver.Minimize(f, batch[b]);
      EXPECT_EQ(s.x[0], one.x[0]);
      EXPECT_EQ(s.x[1], one.x[1]);
      EXPECT_EQ(s.value, one.value);
      EXPECT_EQ(p.num_iterations, one_p.num_iterations);
      EXPECT_TRUE(s.value <= f(batch[b].x));
    }
  }
  TEST_MAIN_END();
}
