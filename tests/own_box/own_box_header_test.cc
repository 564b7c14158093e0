// Lbfgsb::MinimizeBatch(function, states, lower, upper): one box per start state.
//   own_box_header_test refusals   no GPU: what the overload refuses before it reaches the library goes through Fail
//   own_box_header_test solve      GPU: nine states with nine boxes == the nine single SetBounds + Minimize solves
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/lbfgsb.h"
#include "mini_test.h"

using Function = cppoptlib::function::Rosenbrock<>;
using Solver = cppoptlib::solver::Lbfgsb<Function>;
using Vector = Function::VectorType;
using State = Solver::StateType;

constexpr int kN = 5, kBoxes = 9;
constexpr double kMax = 1.7976931348623157e308;

static Vector Filled(double v) {
  Vector x(kN);
  for (int j = 0; j < kN; ++j) x[j] = v;
  return x;
}

// the nine boxes of tests/own_box_cases.py at n = 5, and a start for each
static void Problems(std::vector<State>* states, std::vector<Vector>* lower, std::vector<Vector>* upper) {
  const double lo[kBoxes] = {-kMax, -1.5, -3.0, -kMax, -2.0, 0.9, -1.5, 2.5, -1.0};
  const double hi[kBoxes] = {kMax, 0.8, 3.0, 0.5, 2.0, 0.95, 0.6, 3.5, 1.25};
  for (int b = 0; b < kBoxes; ++b) {
    Vector l = Filled(lo[b]), u = Filled(hi[b]), x(kN);
    for (int j = 0; j < kN; ++j) x[j] = -1.9 + 0.37 * ((7 * b + 3 * j) % 11);   // in [-1.9, 1.8]
    if (b == 4)
      for (int j = 0; j < kN; j += 3) l[j] = u[j] = 0.7;
    if (b == 6)
      for (int j = 0; j < kN; ++j) {
        l[j] = -1.5 + 0.03 * j;
        u[j] = 0.6 + 0.04 * j;
      }
    if (b == 8) {
      x[0] = x[4] = -1.0;
      x[2] = 1.25;
    }
    states->push_back(State(x));
    lower->push_back(l);
    upper->push_back(u);
  }
}

template <class Call>
static std::string Thrown(Call call) {
  try {
    call();
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "(nothing thrown)";
}

static int Refusals() {
  Function f;
  std::vector<State> states;
  std::vector<Vector> lower, upper;
  Problems(&states, &lower, &upper);
  Solver solver;
  {
    std::vector<Vector> fewer(lower.begin(), lower.end() - 1);
    const std::string what = Thrown([&] { solver.MinimizeBatch(f, states, fewer, upper); });
    EXPECT_TRUE(what.find("one lower and one upper bound per start state") != std::string::npos);
  }
  {
    std::vector<Vector> shorter = upper;
    shorter[3] = Vector(kN - 1);
    const std::string what = Thrown([&] { solver.MinimizeBatch(f, states, lower, shorter); });
    EXPECT_TRUE(what.find("bound dimension mismatch") != std::string::npos);
  }
  {
    std::vector<Vector> with_nan = lower;
    with_nan[7][2] = std::nan("");
    const std::string what = Thrown([&] { solver.MinimizeBatch(f, states, with_nan, upper); });
    EXPECT_TRUE(what.find("NaN bound") != std::string::npos);
  }
  EXPECT_TRUE(solver.MinimizeBatch(f, std::vector<State>(), std::vector<Vector>(), std::vector<Vector>()).empty());
  TEST_MAIN_END();
}

static bool SameBits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

static int Solve() {
  Function f;
  std::vector<State> states;
  std::vector<Vector> lower, upper;
  Problems(&states, &lower, &upper);
  for (int arithmetic : {MI355_ARITH_DEFAULT, MI355_ARITH_EXACT}) {
    Solver batched;
    batched.SetArithmetic(arithmetic);
    batched.SetBounds(Filled(-0.1), Filled(0.1));   // the object's own box is not consulted by the overload
    const auto results = batched.MinimizeBatch(f, states, lower, upper);
    EXPECT_EQ(results.size(), size_t(kBoxes));
    int on_bound = 0;
    for (int b = 0; b < kBoxes && results.size() == size_t(kBoxes); ++b) {
      Solver single;
      single.SetArithmetic(arithmetic);
      single.SetBounds(lower[b], upper[b]);
      const auto [state, progress] = single.Minimize(f, states[b]);
      const auto& [bstate, bprogress] = results[b];
      EXPECT_TRUE(SameBits(state.value, bstate.value));
      for (int j = 0; j < kN; ++j) {
        EXPECT_TRUE(SameBits(state.x[j], bstate.x[j]));
        EXPECT_TRUE(SameBits(state.gradient[j], bstate.gradient[j]));
        EXPECT_TRUE(bstate.x[j] >= lower[b][j] && bstate.x[j] <= upper[b][j]);
        on_bound += (bstate.x[j] == lower[b][j] || bstate.x[j] == upper[b][j]);
      }
      EXPECT_TRUE(progress.status == bprogress.status);
      EXPECT_EQ(progress.num_iterations, bprogress.num_iterations);
      EXPECT_EQ(progress.num_function_evaluations, bprogress.num_function_evaluations);
      EXPECT_TRUE(SameBits(progress.x_delta, bprogress.x_delta));
      EXPECT_TRUE(SameBits(progress.f_delta, bprogress.f_delta));
      EXPECT_TRUE(SameBits(progress.gradient_norm, bprogress.gradient_norm));
    }
    EXPECT_TRUE(on_bound >= kBoxes);   // the boxes bind
  }
  TEST_MAIN_END();
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "refusals") return Refusals();
  if (mode == "solve") return Solve();
  std::printf("usage: own_box_header_test refusals | solve\n");
  return 2;
}
