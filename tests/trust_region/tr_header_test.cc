// The scenarios of the reference's src/test/trust_region_newton_test.cc, restated over the drop-in header
// include/cppoptlib/solver/trust_region_newton.h (device solves) with the reference's own bounds.  The functors are
// ours: each states its device twin in one line.  The quartic double well's device functor is the user-objective example,
// built into another library: tests/test_gpu_trust_region.py runs that scenario with the same bounds.
#include <cmath>
#include <cstdio>
#include <vector>

#include "cppoptlib/function.h"
#include "cppoptlib/solver/trust_region_newton.h"
#include "mini_test.h"

using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;
using cppoptlib::function::FunctionState;
using cppoptlib::solver::TrustRegionNewton;
using cppoptlib::solver::TrustRegionNewtonConfig;
namespace twin = cppoptlib::mi355::twin;

// f = sum_i a_i x_i^2 with H = diag(2 a_i): a = (3, 10) is the strictly convex quadratic, (0.5, -0.5) the saddle
template <int A0x2, int A1x2>
class Quadratic : public FunctionCRTP<Quadratic<A0x2, A1x2>, double, DifferentiabilityMode::Second> {
 public:
  using Base = FunctionCRTP<Quadratic<A0x2, A1x2>, double, DifferentiabilityMode::Second>;
  using typename Base::MatrixType;
  using typename Base::ScalarType;
  using typename Base::VectorType;
  static constexpr double a0 = A0x2 / 2.0, a1 = A1x2 / 2.0;
  ScalarType operator()(const VectorType& x, VectorType* grad = nullptr, MatrixType* hess = nullptr) const {
    if (grad) {
      *grad = VectorType(2);
      (*grad)[0] = (2.0 * a0) * x[0];
      (*grad)[1] = (2.0 * a1) * x[1];
    }
    if (hess) {
      *hess = MatrixType(2, 2);
      (*hess)(0, 0) = 2.0 * a0;
      (*hess)(0, 1) = 0.0;
      (*hess)(1, 0) = 0.0;
      (*hess)(1, 1) = 2.0 * a1;
    }
    return (a0 * x[0]) * x[0] + (a1 * x[1]) * x[1];
  }
  auto DeviceTwin() const { return twin::DiagQuadratic({a0, a1}, 0.0); }
};
using StrictlyConvexQuadratic = Quadratic<6, 20>;
using Saddle = Quadratic<1, -1>;

class Rosenbrock2 : public FunctionCRTP<Rosenbrock2, double, DifferentiabilityMode::Second> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* grad = nullptr, MatrixType* hess = nullptr) const {
    const double a = 1 - x[0];
    const double b = x[1] - x[0] * x[0];
    if (grad) {
      *grad = VectorType(2);
      (*grad)[0] = -2 * a - 400 * b * x[0];
      (*grad)[1] = 200 * b;
    }
    if (hess) {
      *hess = MatrixType(2, 2);
      (*hess)(0, 0) = 2 - 400 * b + 800 * x[0] * x[0];
      (*hess)(0, 1) = -400 * x[0];
      (*hess)(1, 0) = -400 * x[0];
      (*hess)(1, 1) = 200;
    }
    return a * a + 100 * b * b;
  }
  auto DeviceTwin() const { return twin::Rosenbrock(); }
};

template <class F>
static typename F::VectorType vec(double a, double b) {
  typename F::VectorType v(2);
  v[0] = a;
  v[1] = b;
  return v;
}
template <class V>
static double dist(const V& a, const V& b) {
  return std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]));
}

int main() {
  {  // StrictlyConvexQuadraticConvergesQuickly
    StrictlyConvexQuadratic f;
    TrustRegionNewton<StrictlyConvexQuadratic> solver;
    solver.stopping_progress.gradient_norm = 1e-10;
    solver.stopping_progress.num_iterations = 20;
    auto [s, p] = solver.Minimize(f, FunctionState(vec<StrictlyConvexQuadratic>(10.0, -5.0)));
    EXPECT_NEAR(s.x[0], 0.0, 1e-8);
    EXPECT_NEAR(s.x[1], 0.0, 1e-8);
    EXPECT_TRUE(p.num_iterations <= 10);
  }
  {  // RosenbrockConvergesFromStandardStart
    Rosenbrock2 f;
    TrustRegionNewton<Rosenbrock2> solver;
    solver.stopping_progress.gradient_norm = 1e-8;
    solver.stopping_progress.num_iterations = 200;
    auto [s, p] = solver.Minimize(f, FunctionState(vec<Rosenbrock2>(-1.2, 1.0)));
    EXPECT_NEAR(s.x[0], 1.0, 1e-5);
    EXPECT_NEAR(s.x[1], 1.0, 1e-5);
    EXPECT_TRUE(p.num_iterations < 80);
  }
  {  // TrustRegionBoundaryExitRespectsRadius: the first accepted step lies on the initial radius (callback replay)
    StrictlyConvexQuadratic f;
    TrustRegionNewtonConfig<double> config;
    config.initial_radius = 0.5;
    TrustRegionNewton<StrictlyConvexQuadratic> solver(config);
    solver.stopping_progress.gradient_norm = 0;
    solver.stopping_progress.num_iterations = 5;
    const auto x0 = vec<StrictlyConvexQuadratic>(5.0, 5.0);
    auto x1 = x0;
    int seen = 0;
    solver.SetCallback([&](const StrictlyConvexQuadratic&, const auto& state, const auto& prog) {
      if (prog.num_iterations == 1 && seen == 0) {
        x1 = state.x;
        ++seen;
      }
    });
    solver.Minimize(f, FunctionState(x0));
    EXPECT_EQ(seen, 1);
    EXPECT_NEAR(dist(x1, x0), config.initial_radius, 1e-10);
  }
  {  // IndefiniteHessianNegativeCurvatureStepIsBounded
    Saddle f;
    TrustRegionNewtonConfig<double> config;
    config.initial_radius = 1.0;
    TrustRegionNewton<Saddle> solver(config);
    solver.stopping_progress.gradient_norm = 0;
    solver.stopping_progress.num_iterations = 5;
    const auto x0 = vec<Saddle>(0.1, 0.5);
    auto x1 = x0;
    int seen = 0;
    solver.SetCallback([&](const Saddle&, const auto& state, const auto& prog) {
      if (prog.num_iterations == 1 && seen == 0) {
        x1 = state.x;
        ++seen;
      }
    });
    auto [s, p] = solver.Minimize(f, FunctionState(x0));
    EXPECT_TRUE(dist(x1, x0) <= config.initial_radius + 1e-10);
    EXPECT_TRUE(dist(x1, x0) > 0.0);
    EXPECT_TRUE(std::isfinite(s.x[0]) && std::isfinite(s.x[1]));
  }
  {  // InteriorNewtonStepReachesClosedFormMinimiser
    StrictlyConvexQuadratic f;
    TrustRegionNewtonConfig<double> config;
    config.initial_radius = 100.0;
    TrustRegionNewton<StrictlyConvexQuadratic> solver(
        cppoptlib::solver::DefaultStoppingSolverProgress<StrictlyConvexQuadratic,
                                                         TrustRegionNewton<StrictlyConvexQuadratic>::StateType>(),
        config);
    solver.stopping_progress.gradient_norm = 1e-12;
    solver.stopping_progress.num_iterations = 5;
    auto [s, p] = solver.Minimize(f, FunctionState(vec<StrictlyConvexQuadratic>(1.0, 1.0)));
    EXPECT_NEAR(s.x[0], 0.0, 1e-10);
    EXPECT_NEAR(s.x[1], 0.0, 1e-10);
    EXPECT_TRUE(p.num_iterations <= 3);
  }
  {  // MaxRadiusCapIsEnforced
    StrictlyConvexQuadratic f;
    TrustRegionNewtonConfig<double> config;
    config.initial_radius = 0.5;
    config.max_radius = 2.0;
    TrustRegionNewton<StrictlyConvexQuadratic> solver(config);
    solver.stopping_progress.gradient_norm = 1e-10;
    solver.stopping_progress.num_iterations = 200;
    auto x_prev = vec<StrictlyConvexQuadratic>(100.0, -100.0);
    double longest = 0.0;
    solver.SetCallback([&](const StrictlyConvexQuadratic&, const auto& state, const auto& prog) {
      if (prog.num_iterations > 0) longest = std::max(longest, dist(state.x, x_prev));
      x_prev = state.x;
    });
    auto [s, p] = solver.Minimize(f, FunctionState(vec<StrictlyConvexQuadratic>(100.0, -100.0)));
    EXPECT_TRUE(longest <= config.max_radius + 1e-10);
    EXPECT_NEAR(s.x[0], 0.0, 1e-8);
    EXPECT_NEAR(s.x[1], 0.0, 1e-8);
    EXPECT_TRUE(p.num_iterations < 150);
  }
  {  // GradientNormStopFires
    StrictlyConvexQuadratic f;
    TrustRegionNewton<StrictlyConvexQuadratic> solver;
    solver.stopping_progress.gradient_norm = 1e-4;
    solver.stopping_progress.num_iterations = 100;
    auto [s, p] = solver.Minimize(f, FunctionState(vec<StrictlyConvexQuadratic>(3.0, 3.0)));
    EXPECT_TRUE(p.status == cppoptlib::solver::Status::GradientNormViolation);
    EXPECT_TRUE(p.num_iterations < 10);
  }
  {  // IterationLimitStopFires
    Rosenbrock2 f;
    TrustRegionNewton<Rosenbrock2> solver;
    solver.stopping_progress.num_iterations = 1;
    solver.stopping_progress.gradient_norm = 1e-16;
    auto [s, p] = solver.Minimize(f, FunctionState(vec<Rosenbrock2>(-1.2, 1.0)));
    EXPECT_TRUE(p.status == cppoptlib::solver::Status::IterationLimit);
  }
  {  // the batched entry point: every start of a small batch reaches the minimiser
    Rosenbrock2 f;
    TrustRegionNewton<Rosenbrock2> solver;
    solver.stopping_progress.gradient_norm = 1e-8;
    std::vector<TrustRegionNewton<Rosenbrock2>::StateType> starts;
    for (int b = 0; b < 16; ++b) starts.emplace_back(vec<Rosenbrock2>(-1.2 + 0.1 * b, 1.0 - 0.05 * b));
    auto out = solver.MinimizeBatch(f, starts);
    EXPECT_EQ(out.size(), size_t(16));
    for (auto& [s, p] : out) {
      EXPECT_NEAR(s.x[0], 1.0, 1e-5);
      EXPECT_NEAR(s.x[1], 1.0, 1e-5);
    }
  }
  TEST_MAIN_END();
}
