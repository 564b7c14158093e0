// The GradientDescent and ConjugatedGradientDescent pairs of the reference's src/test/verify.cc
// (SOLVER_SETUP_CONSERVATIVE(GradientDescent, RosenbrockGradient) and SOLVER_SETUP(ConjugatedGradientDescent,
// RosenbrockGradient): the Far start (15, 8) and the Near start (-1, 2), EXPECT_NEAR(0, f(x*), 1e-4)), restated over the
// drop-in headers include/cppoptlib/solver/gradient_descent.h and conjugated_gradient_descent.h (device solves), plus the
// callback replay and the batched entry point.  The functor is ours: it states its device twin in one line.
#include <cmath>
#include <cstdio>
#include <vector>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/conjugated_gradient_descent.h"
#include "cppoptlib/solver/gradient_descent.h"
#include "mini_test.h"

using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;
using cppoptlib::function::FunctionState;
using cppoptlib::solver::ConjugatedGradientDescent;
using cppoptlib::solver::GradientDescent;
namespace twin = cppoptlib::mi355::twin;

constexpr double PRECISION = 1e-4;

class RosenbrockGradient : public FunctionCRTP<RosenbrockGradient, double, DifferentiabilityMode::First> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* grad = nullptr) const {
    const double t1 = 1 - x[0];
    const double t2 = x[1] - x[0] * x[0];
    if (grad) {
      *grad = VectorType(2);
      (*grad)[0] = -2 * t1 + 200 * t2 * (-2 * x[0]);
      (*grad)[1] = 200 * t2;
    }
    return t1 * t1 + 100 * t2 * t2;
  }
  auto DeviceTwin() const { return twin::Rosenbrock(); }
};

static RosenbrockGradient::VectorType vec(double a, double b) {
  RosenbrockGradient::VectorType v(2);
  v[0] = a;
  v[1] = b;
  return v;
}

template <class Solver>
static void scenario(Solver& solver, double a, double b) {
  RosenbrockGradient f;
  auto [solution, solver_state] = solver.Minimize(f, FunctionState(vec(a, b)));
  EXPECT_TRUE(solver_state.status != cppoptlib::solver::Status::NotStarted);
  EXPECT_NEAR(0.0, f(solution.x), PRECISION);
}

template <class Solver>
static void callback_and_batch() {
  {  // the callback, replayed from the device trace: the start, then every state after an Update, once each
    RosenbrockGradient f;
    auto stop = cppoptlib::solver::DefaultStoppingSolverProgress<RosenbrockGradient, typename Solver::StateType>();
    stop.num_iterations = 40;
    Solver solver(stop);
    int calls = 0, last = -1;
    bool ascending = true;
    double last_value = 0.0;
    solver.SetCallback([&](const RosenbrockGradient&, const auto& state, const auto& prog) {
      ++calls;
      ascending = ascending && static_cast<int>(prog.num_iterations) == last + 1;
      last = static_cast<int>(prog.num_iterations);
      last_value = state.value;
    });
    auto [solution, solver_state] = solver.Minimize(f, FunctionState(vec(-1.0, 2.0)));
    EXPECT_TRUE(ascending);
    EXPECT_EQ(calls, static_cast<int>(solver_state.num_iterations) + 1);
    EXPECT_NEAR(last_value, solution.value, 0.0);
    EXPECT_TRUE(std::isfinite(solution.value));
  }
  {  // a stopping progress handed to the constructor (the reference's `using Superclass::Superclass`)
    RosenbrockGradient f;
    auto stop = cppoptlib::solver::DefaultStoppingSolverProgress<RosenbrockGradient, typename Solver::StateType>();
    stop.num_iterations = 1;
    stop.gradient_norm = 1e-16;
    Solver solver(stop);
    auto [solution, solver_state] = solver.Minimize(f, FunctionState(vec(15.0, 8.0)));
    EXPECT_TRUE(solver_state.status == cppoptlib::solver::Status::IterationLimit);
    EXPECT_TRUE(std::isfinite(solution.value));
  }
  {  // the batched entry point: every start of a small batch gets below its start value
    RosenbrockGradient f;
    Solver solver;
    std::vector<typename Solver::StateType> starts;
    for (int b = 0; b < 16; ++b) starts.emplace_back(vec(0.6 + 0.05 * b, 1.4 - 0.05 * b));
    auto out = solver.MinimizeBatch(f, starts);
    EXPECT_EQ(out.size(), size_t(16));
    for (size_t b = 0; b < out.size(); ++b) EXPECT_TRUE(std::get<0>(out[b]).value <= f(starts[b].x));
  }
}

int main() {
  using GD = GradientDescent<RosenbrockGradient>;
  using CG = ConjugatedGradientDescent<RosenbrockGradient>;
  {  // GradientDescentTest / RosenbrockGradientFar, Near: the conservative stopping preset
    GD far(cppoptlib::solver::ConservativeStoppingSolverProgress<RosenbrockGradient, GD::StateType>());
    scenario(far, 15.0, 8.0);
    GD near(cppoptlib::solver::ConservativeStoppingSolverProgress<RosenbrockGradient, GD::StateType>());
    scenario(near, -1.0, 2.0);
  }
  {  // ConjugatedGradientDescentTest / RosenbrockGradientFar, Near: the default stop
    CG far;
    scenario(far, 15.0, 8.0);
    CG near;
    scenario(near, -1.0, 2.0);
  }
  callback_and_batch<GD>();
  callback_and_batch<CG>();
  TEST_MAIN_END();
}
