// The NewtonDescent pair of the reference's src/test/verify.cc (SOLVER_SETUP(NewtonDescent, RosenbrockFull): the Far
// start (15, 8) and the Near start (-1, 2) under the default stop, EXPECT_NEAR(0, f(x*), 1e-4)), restated over the
// drop-in header include/cppoptlib/solver/newton_descent.h (device solves), plus the callback replay and the batched
// entry point.  The functor is ours: it states its device twin in one line.
#include <cmath>
#include <cstdio>
#include <vector>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/newton_descent.h"
#include "mini_test.h"

using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;
using cppoptlib::function::FunctionState;
using cppoptlib::solver::NewtonDescent;
namespace twin = cppoptlib::mi355::twin;

constexpr double PRECISION = 1e-4;

class RosenbrockFull : public FunctionCRTP<RosenbrockFull, double, DifferentiabilityMode::Second> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* grad = nullptr, MatrixType* hess = nullptr) const {
    const double t1 = 1 - x[0];
    const double t2 = x[1] - x[0] * x[0];
    if (grad) {
      *grad = VectorType(2);
      (*grad)[0] = -2 * t1 + 200 * t2 * (-2 * x[0]);
      (*grad)[1] = 200 * t2;
    }
    if (hess) {
      *hess = MatrixType(2, 2);
      (*hess)(0, 0) = 1200 * x[0] * x[0] - 400 * x[1] + 2;
      (*hess)(0, 1) = -400 * x[0];
      (*hess)(1, 0) = -400 * x[0];
      (*hess)(1, 1) = 200;
    }
    return t1 * t1 + 100 * t2 * t2;
  }
  auto DeviceTwin() const { return twin::Rosenbrock(); }
};

static RosenbrockFull::VectorType vec(double a, double b) {
  RosenbrockFull::VectorType v(2);
  v[0] = a;
  v[1] = b;
  return v;
}

int main() {
  {  // NewtonDescentTest / RosenbrockFarFull
    RosenbrockFull f;
    NewtonDescent<RosenbrockFull> solver;
    auto [solution, solver_state] = solver.Minimize(f, FunctionState(vec(15.0, 8.0)));
    EXPECT_TRUE(solver_state.status != cppoptlib::solver::Status::IterationLimit);
    EXPECT_NEAR(0.0, f(solution.x), PRECISION);
  }
  {  // NewtonDescentTest / RosenbrockNearFull
    RosenbrockFull f;
    NewtonDescent<RosenbrockFull> solver;
    auto [solution, solver_state] = solver.Minimize(f, FunctionState(vec(-1.0, 2.0)));
    EXPECT_TRUE(solver_state.status != cppoptlib::solver::Status::IterationLimit);
    EXPECT_NEAR(0.0, f(solution.x), PRECISION);
  }
  {  // the callback, replayed from the device trace: the start, then every state after an Update, once each
    RosenbrockFull f;
    NewtonDescent<RosenbrockFull> solver;
    int calls = 0, last = -1;
    bool ascending = true;
    double last_value = 0.0;
    solver.SetCallback([&](const RosenbrockFull&, const auto& state, const auto& prog) {
      ++calls;
      ascending = ascending && static_cast<int>(prog.num_iterations) == last + 1;
      last = static_cast<int>(prog.num_iterations);
      last_value = state.value;
    });
    auto [solution, solver_state] = solver.Minimize(f, FunctionState(vec(-1.0, 2.0)));
    EXPECT_TRUE(ascending);
    EXPECT_EQ(calls, static_cast<int>(solver_state.num_iterations) + 1);
    EXPECT_NEAR(last_value, solution.value, 0.0);
    EXPECT_NEAR(0.0, f(solution.x), PRECISION);
  }
  {  // a stopping progress handed to the constructor (the reference's `using Superclass::Superclass`)
    RosenbrockFull f;
    auto stop = cppoptlib::solver::DefaultStoppingSolverProgress<RosenbrockFull,
                                                                 NewtonDescent<RosenbrockFull>::StateType>();
    stop.num_iterations = 1;
    stop.gradient_norm = 1e-16;
    NewtonDescent<RosenbrockFull> solver(stop);
    auto [solution, solver_state] = solver.Minimize(f, FunctionState(vec(15.0, 8.0)));
    EXPECT_TRUE(solver_state.status == cppoptlib::solver::Status::IterationLimit);
    EXPECT_TRUE(std::isfinite(solution.value));
  }
  {  // the batched entry point: every start of a small batch reaches the minimiser
    RosenbrockFull f;
    NewtonDescent<RosenbrockFull> solver;
    std::vector<NewtonDescent<RosenbrockFull>::StateType> starts;
    for (int b = 0; b < 16; ++b) starts.emplace_back(vec(0.6 + 0.05 * b, 1.4 - 0.05 * b));
    auto out = solver.MinimizeBatch(f, starts);
    EXPECT_EQ(out.size(), size_t(16));
    for (auto& [s, p] : out) EXPECT_NEAR(0.0, f(s.x), PRECISION);
  }
  TEST_MAIN_END();
}
