// The four ...OnDevice functions and CheckDeviceTwin of include/cppoptlib/mi355/derivatives.h on the README's quadratic
// (5 x0^2 + 100 x1^2 + 5) and on the 2-D Rosenbrock of the reference's tests: the on-device results must equal the CPU
// twin's in device order (dv_twin.hpp, linked in) bit for bit, and CheckDeviceTwin must report 0 for f, g and H on the
// quadratic, whose device functor states the README's operation order.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cppoptlib/function.h"
#include "cppoptlib/mi355/derivatives.h"
#include "common.h"
#include "mini_test.h"

extern "C" int dv_twin_check(int objective, int n, int64_t B, const double* params, const dv_config* cfg, int order,
                             int width, int elems, const double* x, double* f, double* grad, double* grad_fd,
                             double* hess, double* hess_fd, dv_report* report);

using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;
namespace twin = cppoptlib::mi355::twin;
namespace dv = cppoptlib::mi355::utils;

// README.md quick start, with its Hessian
class Quadratic : public FunctionCRTP<Quadratic, double, DifferentiabilityMode::Second> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* grad = nullptr, MatrixType* hess = nullptr) const {
    if (grad) {
      *grad = VectorType(2);
      (*grad)[0] = 10 * x[0];
      (*grad)[1] = 200 * x[1];
    }
    if (hess) {
      *hess = MatrixType(2, 2);
      (*hess)(0, 0) = 10;
      (*hess)(0, 1) = 0;
      (*hess)(1, 0) = 0;
      (*hess)(1, 1) = 200;
    }
    return 5 * x[0] * x[0] + 100 * x[1] * x[1] + 5;
  }
  auto DeviceTwin() const { return twin::DiagQuadratic({5, 100}, 5); }
};

class Rosenbrock : public FunctionCRTP<Rosenbrock, double, DifferentiabilityMode::Second> {
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

template <class F>
static void against_twin(const F& f, int objective, const double* params, double a, double b, bool hessian_passes) {
  typename F::VectorType x(2);
  x[0] = a;
  x[1] = b;
  const double xs[2] = {a, b};
  for (int accuracy = 0; accuracy <= 3; ++accuracy) {
    dv_config c{accuracy, accuracy, 0.0, 0.0, 0.0, 0.0};
    double tf, tg[2], tgfd[2], th[4], thfd[4];
    dv_report tr;
    EXPECT_EQ(dv_twin_check(objective, 2, 1, params, &c, /*device order*/ 1, /*width*/ 8, 1, xs, &tf, tg, tgfd, th, thfd, &tr), 0);
    typename F::VectorType grad;
    dv::ComputeFiniteGradientOnDevice(f, x, &grad, accuracy);
    EXPECT_TRUE(same_bits(grad[0], tgfd[0]) && same_bits(grad[1], tgfd[1]));
    typename F::MatrixType hess;
    dv::ComputeFiniteHessianOnDevice(f, x, &hess, accuracy);
    for (int j = 0; j < 2; ++j)
      for (int i = 0; i < 2; ++i) EXPECT_TRUE(same_bits(hess(i, j), thfd[j * 2 + i]));
    EXPECT_EQ(dv::IsGradientCorrectOnDevice(f, x, accuracy), tr.gradient_ok == 1);
    EXPECT_EQ(dv::IsHessianCorrectOnDevice(f, x, accuracy), tr.hessian_ok == 1);
  }
  EXPECT_TRUE(dv::IsGradientCorrectOnDevice(f, x));
  if (hessian_passes) EXPECT_TRUE(dv::IsHessianCorrectOnDevice(f, x));
}

int main() {
  const double quadratic_params[3] = {5, 100, 5};
  {
    Quadratic f;
    // f >= 5 everywhere (the README's constant): under the reference's step the second difference carries rounding noise
    // of that size, the zero off-diagonal entry has scale 1, and the verdict is the noise's — equal to the twin's, no more
    against_twin(f, kDvDiagQuadratic, quadratic_params, 0.01, -0.003, false);
    Quadratic::VectorType x(2);
    x[0] = -1.25;
    x[1] = 0.375;
    const dv::DeviceTwinDifference d = dv::CheckDeviceTwin(f, x);
    EXPECT_TRUE(d.hessian_compared);
    EXPECT_NEAR(d.value, 0.0, 0.0);
    EXPECT_NEAR(d.gradient, 0.0, 0.0);
    EXPECT_NEAR(d.hessian, 0.0, 0.0);
  }
  {
    Rosenbrock f;
    // next to the minimiser (f ~ 1e-4), where the reference's step passes a correct Hessian
    against_twin(f, kDvRosenbrock, nullptr, 1.0 + 1.0 / 1024, 1.0 - 1.0 / 1024, true);
    Rosenbrock::VectorType x(2);
    x[0] = -1.0;
    x[1] = 2.0;
    const dv::DeviceTwinDifference d = dv::CheckDeviceTwin(f, x);
    // the host functor above is the reference's test functor: the same operations as the device's in another grouping,
    // so a few units in the last place of values of size <= 1e3
    EXPECT_TRUE(d.value <= 1e-12 && d.gradient <= 1e-11 && d.hessian <= 1e-11);
  }
  TEST_MAIN_END();
}
