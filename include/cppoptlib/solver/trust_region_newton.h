// cppoptlib/solver/trust_region_newton.h — trust-region Newton on the MI355X engine.
//
// Drop-in for the reference's solver/trust_region_newton.h: `TrustRegionNewtonConfig<TScalar>` (same fields and
// defaults) and `TrustRegionNewton<FunctionType>` — one Hessian per outer step, CG-Steihaug on the quadratic model, the
// agreement ratio, the radius update and the in-step rejection loop — under Solver::Minimize (solver/solver.h:181-224).
// Every start state is one problem of a batch solved by the device kernel (csrc/trust_region_kernel.hpp; H(x) n x n in
// LDS from the device functor's hess_full, n <= 64) through mi355_trust_region_newton_minimize_batch_host.  No CPU
// fallback: the function type needs a device twin whose functor has a hess_full (Rosenbrock, DiagQuadratic, user functors
// built with trust_region=True); the library refuses the others.
#ifndef INCLUDE_CPPOPTLIB_SOLVER_TRUST_REGION_NEWTON_H_
#define INCLUDE_CPPOPTLIB_SOLVER_TRUST_REGION_NEWTON_H_

#include <memory>
#include <tuple>
#include <vector>

#include "../../mi355_lbfgs.h"
#include "../mi355/batch_driver.h"
#include "../mi355/context.h"
#include "solver.h"

namespace cppoptlib::solver {

template <typename TScalar>
struct TrustRegionNewtonConfig {
  TScalar initial_radius = TScalar{1};
  TScalar max_radius = TScalar{1e10};
  TScalar acceptance_threshold = TScalar{0.15};
  TScalar shrink_factor = TScalar{0.25};
  TScalar expand_factor = TScalar{2};
  TScalar rho_low = TScalar{0.25};
  TScalar rho_high = TScalar{0.75};
  TScalar cg_forcing_coefficient = TScalar{0.5};
  int cg_max_iterations_floor = 10;
  TScalar min_radius = TScalar{1e-12};
  int rejection_retry_limit = 50;
};

template <typename FunctionType>
class TrustRegionNewton : public Solver<FunctionType, cppoptlib::function::FunctionState<
                                                          typename FunctionType::ScalarType, FunctionType::Dimension>> {
  static_assert(FunctionType::Differentiability == cppoptlib::function::DifferentiabilityMode::Second,
                "TrustRegionNewton requires second-order differentiability: "
                "the Hessian enters the quadratic model explicitly.");
  static_assert(std::is_floating_point<typename FunctionType::ScalarType>::value,
                "ScalarType must be float or double (the MI355X engine computes in fp64 either way)");
  static_assert(cppoptlib::mi355::kHasDeviceTwin<FunctionType>,
                "FunctionType has no device twin (kDeviceObjective / DeviceParams / DeviceTwin, see "
                "cppoptlib/mi355/objectives.h); the MI355X engine has no CPU fallback");
  static_assert(!cppoptlib::mi355::HasPerProblemData<FunctionType>::value,
                "the device TrustRegionNewton kernel is built for objectives without per-problem data");

 public:
  using StateType = cppoptlib::function::FunctionState<typename FunctionType::ScalarType, FunctionType::Dimension>;
  using Superclass = Solver<FunctionType, StateType>;
  using ProgressType = typename Superclass::ProgressType;
  using ScalarType = typename FunctionType::ScalarType;
  using VectorType = typename FunctionType::VectorType;
  using MatrixType = typename FunctionType::MatrixType;
  using Config = TrustRegionNewtonConfig<ScalarType>;

  TrustRegionNewton() : Superclass(), config_() {}
  explicit TrustRegionNewton(Config config) : Superclass(), config_(config) {}
  TrustRegionNewton(const ProgressType& stopping_progress, Config config)
      : Superclass(stopping_progress), config_(config) {}

  const Config& config() const { return config_; }

  void SetContext(std::shared_ptr<cppoptlib::mi355::Context> ctx) { ctx_ = std::move(ctx); }

  // With a callback set the solve is traced on the device and the callback replayed afterwards
  // (cppoptlib/mi355/batch_driver.h); condition_hessian is reported from the host functor's Hessian, and the stopping
  // test on it runs on the device.
  std::tuple<StateType, ProgressType> Minimize(const FunctionType& function,
                                               const StateType& function_state) override {
    return cppoptlib::mi355::MinimizeOneReportingCondition<StateType, ProgressType, VectorType>(
        "TrustRegionNewton", function, function_state, this->HasCallback(), this->step_callback_,
        static_cast<uint64_t>(this->stopping_progress.num_iterations), /*condition_stop=*/0.0,
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
    cppoptlib::mi355::RequireObjective(function, "TrustRegionNewton");
    if (cppoptlib::mi355::CarriesPerProblemData(function))
      cppoptlib::mi355::Fail("TrustRegionNewton: the device kernel is built for objectives without per-problem data");
    const std::vector<double> params = cppoptlib::mi355::ObjectiveParams(function, n);
    mi355_lbfgs_desc d{};
    d.objective = cppoptlib::mi355::PlainObjectiveId(function);
    d.linesearch = MI355_LS_MORE_THUENTE;  // (not used by this solver)
    d.n = n;
    d.m = 1;                               // (not used by this solver)
    d.objective_params = params.empty() ? nullptr : params.data();
    d.n_params = static_cast<int32_t>(params.size());
    d.trace = trace;
    d.hessian_condition_stop = static_cast<double>(this->stopping_progress.condition_hessian);
    d.stop = this->stopping_progress.ToDeviceStop();
    mi355_trust_region_config c;
    c.initial_radius = static_cast<double>(config_.initial_radius);
    c.max_radius = static_cast<double>(config_.max_radius);
    c.acceptance_threshold = static_cast<double>(config_.acceptance_threshold);
    c.shrink_factor = static_cast<double>(config_.shrink_factor);
    c.expand_factor = static_cast<double>(config_.expand_factor);
    c.rho_low = static_cast<double>(config_.rho_low);
    c.rho_high = static_cast<double>(config_.rho_high);
    c.cg_forcing_coefficient = static_cast<double>(config_.cg_forcing_coefficient);
    c.cg_max_iterations_floor = config_.cg_max_iterations_floor;
    c.min_radius = static_cast<double>(config_.min_radius);
    c.rejection_retry_limit = config_.rejection_retry_limit;
    cppoptlib::mi355::Check(mi355_trust_region_newton_minimize_batch_host(ctx_->get(), &d, &c, B, x0, x, f, g, progress),
                            "mi355_trust_region_newton_minimize_batch_host");
  }

 private:
  Config config_;
  std::shared_ptr<cppoptlib::mi355::Context> ctx_;
};

}  // namespace cppoptlib::solver
#endif  // INCLUDE_CPPOPTLIB_SOLVER_TRUST_REGION_NEWTON_H_
