// cppoptlib/solver/nelder_mead.h — Nelder-Mead on the MI355X engine.
//
// Drop-in for the reference's solver/nelder_mead.h: `NelderMead<FunctionType>`, the derivative-free simplex method
// (ordering, degeneracy restart, centroid, reflection / expansion / contraction / shrink) under Solver::Minimize
// (solver/solver.h:181-224).  As in the reference the default constructor takes the conservative stopping preset with
// x_delta_violations = 5.  Every start state is one problem of a batch solved by the device kernel
// (csrc/nelder_mead_kernel.hpp; the simplex n x (n + 1) in LDS, n <= 64) through mi355_nelder_mead_minimize_batch_host.
// A None-mode function type runs in value mode (no gradient anywhere); a First- or Second-mode one in first mode (value
// and gradient at the returned vertex once per step, the gradient test of Progress::Update on).  No CPU fallback: the
// function type needs a device twin (Rosenbrock, DiagQuadratic, user functors built with nelder_mead=True).
#ifndef INCLUDE_CPPOPTLIB_SOLVER_NELDER_MEAD_H_
#define INCLUDE_CPPOPTLIB_SOLVER_NELDER_MEAD_H_

#include <memory>
#include <tuple>
#include <vector>

#include "../../mi355_lbfgs.h"
#include "../mi355/batch_driver.h"
#include "../mi355/context.h"
#include "solver.h"

namespace cppoptlib::solver {

template <typename FunctionType>
class NelderMead : public Solver<FunctionType, cppoptlib::function::FunctionState<typename FunctionType::ScalarType,
                                                                                   FunctionType::Dimension>> {
  static_assert(std::is_floating_point<typename FunctionType::ScalarType>::value,
                "ScalarType must be float or double (the MI355X engine computes in fp64 either way)");
  static_assert(cppoptlib::mi355::kHasDeviceTwin<FunctionType>,
                "FunctionType has no device twin (kDeviceObjective / DeviceParams / DeviceTwin, see "
                "cppoptlib/mi355/objectives.h); the MI355X engine has no CPU fallback");
  static_assert(!cppoptlib::mi355::HasPerProblemData<FunctionType>::value,
                "the device NelderMead kernel is built for objectives without per-problem data");

 public:
  using StateType = cppoptlib::function::FunctionState<typename FunctionType::ScalarType, FunctionType::Dimension>;
  using Superclass = Solver<FunctionType, StateType>;
  using ProgressType = typename Superclass::ProgressType;
  using ScalarType = typename FunctionType::ScalarType;
  using VectorType = typename FunctionType::VectorType;
  using MatrixType = typename FunctionType::MatrixType;

  // the reference's coefficients (const members there, nelder_mead.h:58-64)
  const ScalarType rho_ = 1.0;
  const ScalarType xi_ = 20.0;
  const ScalarType gamma_ = 0.1;
  const ScalarType sigma_ = 0.5;
  const ScalarType degenerate_tol_ = 1e-8;

  // nelder_mead.h:87-91: derivative-free, so x_delta / f_delta alone decide; five strikes, the wider plateau window
  NelderMead() : Superclass(ConservativeStoppingSolverProgress<FunctionType, StateType>()) {
    this->stopping_progress.x_delta_violations = 5;
  }
  explicit NelderMead(const ProgressType& stopping_progress) : Superclass(stopping_progress) {}  // `using Superclass::Superclass`

  void SetContext(std::shared_ptr<cppoptlib::mi355::Context> ctx) { ctx_ = std::move(ctx); }

  // With a callback set the solve is traced on the device and the callback replayed afterwards
  // (cppoptlib/mi355/batch_driver.h).
  std::tuple<StateType, ProgressType> Minimize(const FunctionType& function,
                                               const StateType& function_state) override {
    return cppoptlib::mi355::MinimizeOne<StateType, ProgressType, VectorType>(
        function, function_state, this->HasCallback(), this->step_callback_,
        static_cast<uint64_t>(this->stopping_progress.num_iterations),
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
    cppoptlib::mi355::RequireObjective(function, "NelderMead");
    if (cppoptlib::mi355::CarriesPerProblemData(function))
      cppoptlib::mi355::Fail("NelderMead: the device kernel is built for objectives without per-problem data");
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
    mi355_nelder_mead_config c;
    c.rho = static_cast<double>(rho_);
    c.xi = static_cast<double>(xi_);
    c.gamma = static_cast<double>(gamma_);
    c.sigma = static_cast<double>(sigma_);
    c.degenerate_tol = static_cast<double>(degenerate_tol_);
    c.mode = (FunctionType::Differentiability == cppoptlib::function::DifferentiabilityMode::None) ? MI355_NM_MODE_VALUE
                                                                                                   : MI355_NM_MODE_FIRST;
    cppoptlib::mi355::Check(mi355_nelder_mead_minimize_batch_host(ctx_->get(), &d, &c, B, x0, x, f, g, progress),
                            "mi355_nelder_mead_minimize_batch_host");
  }

 private:
  std::shared_ptr<cppoptlib::mi355::Context> ctx_;
};

}  // namespace cppoptlib::solver
#endif  // INCLUDE_CPPOPTLIB_SOLVER_NELDER_MEAD_H_
