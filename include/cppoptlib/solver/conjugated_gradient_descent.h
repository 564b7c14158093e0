// cppoptlib/solver/conjugated_gradient_descent.h — conjugated gradient descent on the MI355X engine.
//
// Drop-in for the reference's solver/conjugated_gradient_descent.h: `ConjugatedGradientDescent<FunctionType>` — d = -g at the first step,
// then beta = (g.g) / (g_prev.g_prev) and d = -g + beta d, the backtracking search Armijo<F, 1> from alpha = 1 (the
// reference's linesearch/armijo.h; the search runs on the device and no header of linesearch/ is needed here), x + alpha d —
// under Solver::Minimize (solver/solver.h:181-224).  Every start state is one problem of a batch solved by the device
// kernel (csrc/first_order_kernel.hpp; x, g and the direction in registers, n <= 256) through
// mi355_conjugated_gradient_descent_minimize_batch_host.  No CPU fallback: the function type needs a device twin without per-problem
// data (Rosenbrock, DiagQuadratic, user functors built with first_order=True); the library refuses the others.
#ifndef INCLUDE_CPPOPTLIB_SOLVER_CONJUGATED_GRADIENT_DESCENT_H_
#define INCLUDE_CPPOPTLIB_SOLVER_CONJUGATED_GRADIENT_DESCENT_H_

#include <memory>
#include <tuple>
#include <vector>

#include "../../mi355_lbfgs.h"
#include "../mi355/batch_driver.h"
#include "../mi355/context.h"
#include "solver.h"

namespace cppoptlib::solver {

template <typename FunctionType>
class ConjugatedGradientDescent : public Solver<FunctionType, cppoptlib::function::FunctionState<
                                                      typename FunctionType::ScalarType, FunctionType::Dimension>> {
  static_assert(FunctionType::Differentiability == cppoptlib::function::DifferentiabilityMode::First ||
                    FunctionType::Differentiability == cppoptlib::function::DifferentiabilityMode::Second,
                "ConjugatedGradientDescent only supports first- or second-order "
                "differentiable functions");
  static_assert(std::is_floating_point<typename FunctionType::ScalarType>::value,
                "ScalarType must be float or double (the MI355X engine computes in fp64 either way)");
  static_assert(cppoptlib::mi355::kHasDeviceTwin<FunctionType>,
                "FunctionType has no device twin (kDeviceObjective / DeviceParams / DeviceTwin, see "
                "cppoptlib/mi355/objectives.h); the MI355X engine has no CPU fallback");
  static_assert(!cppoptlib::mi355::HasPerProblemData<FunctionType>::value,
                "the device ConjugatedGradientDescent kernel is built for objectives without per-problem data");

 public:
  using StateType = cppoptlib::function::FunctionState<typename FunctionType::ScalarType, FunctionType::Dimension>;
  using Superclass = Solver<FunctionType, StateType>;
  using ProgressType = typename Superclass::ProgressType;
  using ScalarType = typename FunctionType::ScalarType;
  using VectorType = typename FunctionType::VectorType;

  using Superclass::Superclass;

  void SetContext(std::shared_ptr<cppoptlib::mi355::Context> ctx) { ctx_ = std::move(ctx); }

  // With a callback set the solve is traced on the device and the callback replayed afterwards
  // (cppoptlib/mi355/batch_driver.h); a Second-mode function's condition_hessian is reported from the host functor's
  // Hessian, and a stopping threshold on it is refused.
  std::tuple<StateType, ProgressType> Minimize(const FunctionType& function,
                                               const StateType& function_state) override {
    return cppoptlib::mi355::MinimizeOneReportingCondition<StateType, ProgressType, VectorType>(
        "ConjugatedGradientDescent", function, function_state, this->HasCallback(), this->step_callback_,
        static_cast<uint64_t>(this->stopping_progress.num_iterations),
        static_cast<double>(this->stopping_progress.condition_hessian),
        [&](int n, int64_t B, const double* x0, double* x, double* f, double* g, mi355_lbfgs_progress* prog,
            const mi355_lbfgs_trace* trace) { MinimizeBatchRaw(function, n, B, x0, x, f, g, prog, trace); });
  }

  // Solves every start state independently in one kernel launch.
  std::vector<std::tuple<StateType, ProgressType>> MinimizeBatch(const FunctionType& function,
                                                                 const std::vector<StateType>& states) {
    const int64_t B = static_cast<int64_t>(states.size());
    if (B == 0) return {};
    const int n = static_cast<int>(states[0].x.size());
    const std::vector<double> x0 = cppoptlib::mi355::PackStates(states, n);
    std::vector<double> x(x0.size()), g(x0.size()), f(static_cast<size_t>(B));
    std::vector<mi355_lbfgs_progress> prog(static_cast<size_t>(B));
    MinimizeBatchRaw(function, n, B, x0.data(), x.data(), f.data(), g.data(), prog.data());
    return cppoptlib::mi355::UnpackResults<StateType, ProgressType, VectorType>(n, B, x, f, g, prog);
  }

  void MinimizeBatchRaw(const FunctionType& function, int n, int64_t B, const double* x0, double* x, double* f,
                        double* g, mi355_lbfgs_progress* progress, const mi355_lbfgs_trace* trace = nullptr) {
    if (!ctx_) ctx_ = cppoptlib::mi355::Context::Default();
    cppoptlib::mi355::RequireObjective(function, "ConjugatedGradientDescent");
    if (cppoptlib::mi355::CarriesPerProblemData(function))
      cppoptlib::mi355::Fail("ConjugatedGradientDescent: the device kernel is built for objectives without per-problem data");
    const std::vector<double> params = cppoptlib::mi355::ObjectiveParams(function, n);
    mi355_lbfgs_desc d{};
    d.objective = cppoptlib::mi355::PlainObjectiveId(function);
    d.linesearch = MI355_LS_MORE_THUENTE;  // (not used by this solver)
    d.n = n;
    d.m = 1;                               // (not used by this solver)
    d.objective_params = params.empty() ? nullptr : params.data();
    d.n_params = static_cast<int32_t>(params.size());
    d.trace = trace;
    d.stop = this->stopping_progress.ToDeviceStop();
    cppoptlib::mi355::Check(
        // the reference's Armijo constants (constexpr there): NULL = the defaults of mi355_armijo_default_config
        mi355_conjugated_gradient_descent_minimize_batch_host(ctx_->get(), &d, nullptr, B, x0, x, f, g, progress),
        "mi355_conjugated_gradient_descent_minimize_batch_host");
  }

 private:
  std::shared_ptr<cppoptlib::mi355::Context> ctx_;
};

}  // namespace cppoptlib::solver
#endif  // INCLUDE_CPPOPTLIB_SOLVER_CONJUGATED_GRADIENT_DESCENT_H_
