// cppoptlib/mi355/derivatives.h — the derivative check of utils/derivatives.h run on the DEVICE twin of a function.
//
// cppoptlib::utils::ComputeFiniteGradient / ComputeFiniteHessian / IsGradientCorrect / IsHessianCorrect
// (../utils/derivatives.h) evaluate the HOST operator().  What a solver of this library runs is the function's device
// twin: a hand-written HIP functor tied to the host function by one DeviceTwin() line (or a kDeviceObjective id).  The
// four functions below take the reference's argument lists, resolve the twin as the solvers do and run the same
// arithmetic on the device through mi355_check_derivatives_batch_host (csrc/derivative_check_kernel.hpp): the finite
// differences are built from the DEVICE functor's values and compared with the DEVICE functor's gradient / Hessian.
// CheckDeviceTwin compares the device functor's analytic outputs with the host operator()'s: the direct test of a
// DeviceTwin() line.
//
// No CPU fallback: a function without a device twin, or with per-problem data, is refused.  n <= 256 for the gradient,
// n <= 64 for the Hessian, functors with a hess_full for the analytic Hessian (Rosenbrock, DiagQuadratic, user functors
// built with derivatives=True).  The optional last argument selects the engine context (default: the process's).
// Compiles with plain g++ and with -fno-exceptions (failures abort there, as everywhere in these headers).
#ifndef INCLUDE_CPPOPTLIB_MI355_DERIVATIVES_H_
#define INCLUDE_CPPOPTLIB_MI355_DERIVATIVES_H_

#include <cmath>
#include <cstddef>
#include <memory>
#include <vector>

#include "../../mi355_lbfgs.h"
#include "../function_base.h"
#include "batch_driver.h"
#include "context.h"

namespace cppoptlib::mi355::utils {

namespace detail {
// one point through mi355_check_derivatives_batch_host; null outputs are not computed
template <class FunctionType, class VectorType>
void CheckOnePoint(const char* where, const FunctionType& function, const VectorType& x0,
                   const mi355_derivative_config& config, std::shared_ptr<Context> ctx, double* f, double* grad,
                   double* grad_fd, double* hess, double* hess_fd, mi355_derivative_report* report) {
  static_assert(kHasDeviceTwin<FunctionType>,
                "FunctionType has no device twin (kDeviceObjective / DeviceParams / DeviceTwin, see "
                "cppoptlib/mi355/objectives.h); the MI355X engine has no CPU fallback");
  if (!ctx) ctx = Context::Default();
  RequireObjective(function, where);
  if (CarriesPerProblemData(function))
    Fail(std::string(where) + ": the derivative check is built for objectives without per-problem data");
  const int n = static_cast<int>(x0.size());
  const std::vector<double> params = ObjectiveParams(function, n);
  std::vector<double> x(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) x[static_cast<size_t>(i)] = static_cast<double>(x0[i]);
  mi355_lbfgs_desc d{};
  d.objective = PlainObjectiveId(function);
  d.n = n;
  d.m = 1;   // (not read)
  d.objective_params = params.empty() ? nullptr : params.data();
  d.n_params = static_cast<int32_t>(params.size());
  Check(mi355_check_derivatives_batch_host(ctx->get(), &d, &config, 1, x.data(), f, grad, grad_fd, hess, hess_fd, report),
        where);
}
inline mi355_derivative_config ConfigWithAccuracy(int accuracy) {
  mi355_derivative_config c;
  mi355_derivative_default_config(&c);
  c.gradient_accuracy = accuracy;
  c.hessian_accuracy = accuracy;
  return c;
}
}  // namespace detail

// utils::ComputeFiniteGradient on the device twin's values
template <class FunctionType>
void ComputeFiniteGradientOnDevice(
    const FunctionType& function,
    const Vector<typename FunctionType::ScalarType, cppoptlib::function::kDynamicDimension>& x0,
    Vector<typename FunctionType::ScalarType, cppoptlib::function::kDynamicDimension>* grad, const int accuracy = 0,
    std::shared_ptr<Context> ctx = nullptr) {
  using Scalar = typename FunctionType::ScalarType;
  const std::ptrdiff_t n = x0.size();
  std::vector<double> fd(static_cast<size_t>(n));
  detail::CheckOnePoint("ComputeFiniteGradientOnDevice", function, x0, detail::ConfigWithAccuracy(accuracy), ctx,
                        nullptr, nullptr, fd.data(), nullptr, nullptr, nullptr);
  grad->resize(n);
  for (std::ptrdiff_t d = 0; d < n; ++d) (*grad)[d] = static_cast<Scalar>(fd[static_cast<size_t>(d)]);
}

// utils::ComputeFiniteHessian on the device twin's values
template <class FunctionType>
void ComputeFiniteHessianOnDevice(
    const FunctionType& function,
    const Vector<typename FunctionType::ScalarType, cppoptlib::function::kDynamicDimension>& x0,
    SquareMatrix<typename FunctionType::ScalarType, cppoptlib::function::kDynamicDimension>* hessian, int accuracy = 0,
    std::shared_ptr<Context> ctx = nullptr) {
  using Scalar = typename FunctionType::ScalarType;
  using MatrixType = SquareMatrix<Scalar, cppoptlib::function::kDynamicDimension>;
  const std::ptrdiff_t n = x0.size();
  std::vector<double> fd(static_cast<size_t>(n * n));
  detail::CheckOnePoint("ComputeFiniteHessianOnDevice", function, x0, detail::ConfigWithAccuracy(accuracy), ctx,
                        nullptr, nullptr, nullptr, nullptr, fd.data(), nullptr);
  *hessian = MatrixType(n, n);
  for (std::ptrdiff_t j = 0; j < n; ++j)
    for (std::ptrdiff_t i = 0; i < n; ++i) (*hessian)(i, j) = static_cast<Scalar>(fd[static_cast<size_t>(j * n + i)]);
}

// utils::IsGradientCorrect: the device functor's gradient against the finite differences of its values
template <class FunctionType>
bool IsGradientCorrectOnDevice(const FunctionType& function, const typename FunctionType::VectorType& x0,
                               int accuracy = 3, std::shared_ptr<Context> ctx = nullptr) {
  mi355_derivative_report report{};
  detail::CheckOnePoint("IsGradientCorrectOnDevice", function, x0, detail::ConfigWithAccuracy(accuracy), ctx, nullptr,
                        nullptr, nullptr, nullptr, nullptr, &report);
  if (report.gradient_ok < 0) Fail("IsGradientCorrectOnDevice: the device functor has no gradient to check");
  return report.gradient_ok == 1;
}

// utils::IsHessianCorrect: the device functor's hess_full against the finite differences of its values
template <class FunctionType>
bool IsHessianCorrectOnDevice(const FunctionType& function, const typename FunctionType::VectorType& x0,
                              int accuracy = 3, std::shared_ptr<Context> ctx = nullptr) {
  const std::ptrdiff_t n = x0.size();
  std::vector<double> hess(static_cast<size_t>(n * n));   // (asking for it is what asks for the Hessian check)
  mi355_derivative_report report{};
  detail::CheckOnePoint("IsHessianCorrectOnDevice", function, x0, detail::ConfigWithAccuracy(accuracy), ctx, nullptr,
                        nullptr, nullptr, hess.data(), nullptr, &report);
  return report.hessian_ok == 1;
}

// max |host - device| over the value, the gradient and (Second-mode functions) the Hessian at x0
struct DeviceTwinDifference {
  double value = 0.0, gradient = 0.0, hessian = 0.0;
  bool hessian_compared = false;
};
template <class FunctionType>
DeviceTwinDifference CheckDeviceTwin(const FunctionType& function, const typename FunctionType::VectorType& x0,
                                     std::shared_ptr<Context> ctx = nullptr) {
  using VectorType = typename FunctionType::VectorType;
  constexpr bool kSecond = FunctionType::Differentiability == cppoptlib::function::DifferentiabilityMode::Second;
  const std::ptrdiff_t n = x0.size();
  double f_device = 0.0;
  std::vector<double> g_device(static_cast<size_t>(n)), h_device(kSecond ? static_cast<size_t>(n * n) : 0);
  detail::CheckOnePoint("CheckDeviceTwin", function, x0, detail::ConfigWithAccuracy(3), ctx, &f_device, g_device.data(),
                        nullptr, kSecond ? h_device.data() : nullptr, nullptr, nullptr);
  DeviceTwinDifference out;
  auto widen = [](double& m, double d) {
    d = std::fabs(d);
    if (m < d || d != d) m = d;   // (a NaN difference is reported, not dropped)
  };
  VectorType g_host;
  if constexpr (kSecond) {
    typename FunctionType::MatrixType h_host;
    widen(out.value, static_cast<double>(function(x0, &g_host, &h_host)) - f_device);
    for (std::ptrdiff_t j = 0; j < n; ++j)
      for (std::ptrdiff_t i = 0; i < n; ++i)
        widen(out.hessian, static_cast<double>(h_host(i, j)) - h_device[static_cast<size_t>(j * n + i)]);
    out.hessian_compared = true;
  } else {
    widen(out.value, static_cast<double>(function(x0, &g_host)) - f_device);
  }
  for (std::ptrdiff_t d = 0; d < n; ++d) widen(out.gradient, static_cast<double>(g_host[d]) - g_device[static_cast<size_t>(d)]);
  return out;
}

}  // namespace cppoptlib::mi355::utils
#endif  // INCLUDE_CPPOPTLIB_MI355_DERIVATIVES_H_
