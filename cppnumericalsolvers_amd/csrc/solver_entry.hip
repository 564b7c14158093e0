// solver_entry.hip — the C entry points of TrustRegionNewton, NewtonDescent, NelderMead, GradientDescent and
// ConjugatedGradientDescent (include/mi355_lbfgs.h).  minimize_batch() is the one sequence all five run: neutralise the
// desc fields that mean nothing to them, the Hessian fields, the n limit, validate(), the arithmetic, the objective, the
// lane mapping, the config, B == 0, the pointers, then the device (parameter blob, kernel arguments, trace, dispatch).  A
// Solver record and two lambdas per entry point hold what differs; the one difference in order is NelderMead's objective
// check, which also runs before validate() (ObjectiveCheck).  No kernel lives here.
#include "engine_internal.hpp"
#include "lbfgs_f32_config.hpp"

namespace {
using namespace mi355;

// the inputs and outputs of one call, as the entry points receive them
struct Batch {
  int64_t B;
  const double* x0;
  double *x_out, *f_out, *g_out;
  mi355_lbfgs_progress* progress_out;
  void* stream;
};

enum HessianFields {
  kHessianFromFunctor,   // H(x) is the functor's hess_full: hessian_diagonal must be NULL, hessian_condition_stop is read
  kHessianIgnored,       // a derivative-free solver: every Hessian field is cleared
  kHessianUnused,        // a first-order solver: cleared too, but hessian_condition_stop must be 0 (the test is not run)
};

enum Mapping {
  kOnePerLane,            // lanes_covering: 8, 16, 32 or 64 lanes at one coordinate per lane
  kOnePerLane64Over32,    // ... where the library's own choice of 32 lanes becomes 64
  kUpToFourPerLane,       // first_order_mapping
};
// Where the solver answers an objective it has no kernel for.  validate() calls an id that no built-in has, and a user id
// this library has no entry for, "unknown objective id" (MI355_ERR_UNSUPPORTED); NelderMead has always answered those
// itself, with its own code and the text that names the build key, and keeps doing so.
enum ObjectiveCheck { kObjectiveAfterValidate, kObjectiveBeforeValidate };

// What differs between the solvers, but for the config and the dispatch call.  The texts follow the solver's name.  Every
// member but the texts has a type of its own, and the records below name the texts, so a transposed entry does not compile.
struct Solver {
  const char* name;
  int max_n;
  const char* beyond_max_n;
  int not_built;                 // the code of the "not built" refusals: the n limit, the arithmetic, the objective
  HessianFields hessian;
  UserSolver user_slot;          // the registry slot of its kernels on a user functor ...
  const char* no_user_kernel;    // ... the refusal of a user objective without them, and of any other objective
  const char* no_builtin_kernel;
  ObjectiveCheck objective_check;
  Mapping mapping;
};

const char kDeviceHessianOnly[] =
    " is built for objectives with a device Hessian (hess_full): Rosenbrock, DiagQuadratic and user functors; the ridge "
    "forms, the augmented-Lagrangian composite and sum / product records have none";
const Solver kTrustRegionNewton = {
    "TrustRegionNewton", kHessianConditionMaxN,
    /*beyond_max_n=*/" is built for n <= 64 (H is n x n in LDS per problem)",
    MI355_ERR_UNSUPPORTED, kHessianFromFunctor, kUserTrustRegion,
    /*no_user_kernel=*/": this library holds no trust-region kernel for this user objective (build it with "
                       "trust_region=True and a functor that defines hess_full)",
    /*no_builtin_kernel=*/kDeviceHessianOnly, kObjectiveAfterValidate, kOnePerLane};
const Solver kNelderMead = {
    "NelderMead", 64,
    /*beyond_max_n=*/" is built for n <= 64 (the simplex is n x (n + 1) in LDS per problem)",
    MI355_ERR_INVALID_ARGUMENT, kHessianIgnored, kUserNelderMead,
    /*no_user_kernel=*/": this library holds no Nelder-Mead kernel for this user objective (build it with nelder_mead=True "
                       "and a functor that defines value)",
    /*no_builtin_kernel=*/" is built for Rosenbrock, DiagQuadratic and user functors built with nelder_mead=True",
    kObjectiveBeforeValidate, kOnePerLane};
// the library's choice of lanes is the padded width, except 16 < n <= 32: 64 lanes measured faster there (one problem per
// wavefront halves the LDS per wavefront; profiles/newton_descent_bench.jsonl)
const Solver kNewtonDescent = {
    "NewtonDescent", 64,
    /*beyond_max_n=*/" is built for n <= 64 (H and its LU are n x n in LDS per problem)",
    MI355_ERR_UNSUPPORTED, kHessianFromFunctor, kUserNewtonDescent,
    /*no_user_kernel=*/": this library holds no Newton-descent kernel for this user objective (build it with "
                       "newton_descent=True and a functor that defines hess_full)",
    /*no_builtin_kernel=*/kDeviceHessianOnly, kObjectiveAfterValidate, kOnePerLane64Over32};
Solver first_order_solver(const char* name) {
  return {name, MI355_LBFGS_MAX_N,
          /*beyond_max_n=*/" is built for n <= 256 (x, g and d in registers, up to four coordinates per lane)",
          MI355_ERR_UNSUPPORTED, kHessianUnused, kUserFirstOrder,
          /*no_user_kernel=*/": this library holds no first-order kernel for this user objective (build it with "
                             "first_order=True)",
          /*no_builtin_kernel=*/" is built for objectives without LDS data: Rosenbrock, DiagQuadratic and user functors "
                                "built with first_order=True; not the ridge forms or the augmented-Lagrangian composite",
          kObjectiveAfterValidate, kUpToFourPerLane};
}

int refuse(int code, const Solver& s, const char* text) { return fail(code, std::string(s.name) + text); }

// lanes per problem of a one-coordinate-per-lane solver (n <= 64): the padded width of n where the caller leaves it to the
// library (0), else the caller's, which must be one of 8 / 16 / 32 / 64 and cover n; 0: it is not
int lanes_covering(int requested, int n) {
  if (requested == 0) {
    int W = 8;
    while (W < n) W <<= 1;
    return W;
  }
  const bool built = requested == 8 || requested == 16 || requested == 32 || requested == 64;
  return (built && requested >= n) ? requested : 0;
}

int one_per_lane_mapping(const Solver& s, const mi355_lbfgs_desc& desc, int& W, int& E) {
  if (desc.elems_per_lane != 0 && desc.elems_per_lane != 1)
    return refuse(MI355_ERR_INVALID_ARGUMENT, s, ": one coordinate per lane (elems_per_lane 0 or 1)");
  W = lanes_covering(desc.lanes_per_problem, desc.n);
  E = 1;
  if (W == 0) return refuse(MI355_ERR_INVALID_ARGUMENT, s, ": lanes_per_problem must be 8, 16, 32 or 64 and cover n");
  if (s.mapping == kOnePerLane64Over32 && desc.lanes_per_problem == 0 && W == 32) W = 64;
  return MI355_OK;
}

// the padded width at one coordinate per lane up to 64, then 64 lanes at two and four
int first_order_mapping(const Solver& s, const mi355_lbfgs_desc& desc, int& W, int& E) {
  W = desc.lanes_per_problem;
  E = desc.elems_per_lane;
  if (W == 0) {
    if (E != 0) return refuse(MI355_ERR_INVALID_ARGUMENT, s, ": elems_per_lane needs an explicit lanes_per_problem");
    W = 8;
    while (W < desc.n && W < 64) W <<= 1;
  } else if (!(W == 8 || W == 16 || W == 32 || W == 64)) {
    return refuse(MI355_ERR_INVALID_ARGUMENT, s, ": lanes_per_problem must be 0, 8, 16, 32 or 64");
  }
  if (E == 0) E = (desc.n <= W) ? 1 : ((desc.n <= 2 * W) ? 2 : 4);
  if (!(E == 1 || ((E == 2 || E == 4) && W == 64)) || W * E < desc.n)
    return refuse(MI355_ERR_INVALID_ARGUMENT, s,
                  ": the mapping must cover n with 8, 16, 32 or 64 lanes at one coordinate per lane, or 64 lanes at two "
                  "or four");
  return MI355_OK;
}

// the kernel arguments every one of these solvers fills the same way (m means nothing to them; the parameter blob is
// the one upload_params left in the context)
SolveArgs solver_args(const mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc& desc, const Batch& io) {
  SolveArgs args;
  std::memset(&args, 0, sizeof(args));
  args.x0 = io.x0;
  args.x_out = io.x_out;
  args.f_out = io.f_out;
  args.g_out = io.g_out;
  args.progress_out = io.progress_out;
  args.obj_params = ctx->params_dev;
  args.per_problem = desc.per_problem_data;
  args.per_problem_stride = desc.per_problem_stride;
  args.B = io.B;
  args.n = desc.n;
  args.m = 1;
  args.stop = desc.stop;
  args.hess_from_functor = desc.hessian_from_functor;            // (both zero unless s.hessian == kHessianFromFunctor)
  args.hessian_condition_stop = desc.hessian_condition_stop;
  return args;
}

// configure(dc): the public config (or its defaults) -> the device config, with the checks that belong to it;
// dispatch(W, E, objective, args, dc, stream): the solver's dispatch unit
template <class DeviceConfig, class Configure, class Dispatch>
int minimize_batch(const Solver& s, mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc_in, const Batch& io,
                   Configure configure, Dispatch dispatch) {
  if (!desc_in) return fail(MI355_ERR_INVALID_ARGUMENT, "null desc");
  mi355_lbfgs_desc desc = *desc_in;   // m, the line search and the history placement mean nothing to these solvers
  desc.m = 1;
  desc.linesearch = MI355_LS_MORE_THUENTE;
  desc.history_placement = 0;
  if (s.hessian == kHessianFromFunctor) {
    if (desc.hessian_diagonal != nullptr)
      return refuse(MI355_ERR_INVALID_ARGUMENT, s, ": H(x) comes from the device functor (hessian_diagonal NULL)");
    desc.hessian_from_functor = 1;
  } else {
    desc.hessian_diagonal = nullptr;
    desc.hessian_from_functor = 0;
    if (s.hessian == kHessianIgnored) desc.hessian_condition_stop = 0.0;
    if (desc.hessian_condition_stop != 0.0)
      return refuse(MI355_ERR_INVALID_ARGUMENT, s,
                    ": the condition_hessian test is not evaluated (hessian_condition_stop must be 0)");
  }
  if (desc.n > s.max_n) return refuse(s.not_built, s, s.beyond_max_n);
  const bool user = desc.objective >= MI355_OBJ_USER_FIRST;
  const bool has_kernel = desc.objective == MI355_OBJ_ROSENBROCK || desc.objective == MI355_OBJ_DIAG_QUADRATIC ||
                          (user && user_solver(desc.objective, s.user_slot) != nullptr);
  if (!has_kernel && s.objective_check == kObjectiveBeforeValidate)
    return refuse(s.not_built, s, user ? s.no_user_kernel : s.no_builtin_kernel);
  int rc = validate(ctx, &desc, io.B);
  if (rc != MI355_OK) return rc;
  if (desc.arithmetic == MI355_ARITH_FMA)
    return refuse(s.not_built, s, " is built for the exact arithmetic only (no MI355_ARITH_FMA)");
  if (!has_kernel) return refuse(s.not_built, s, user ? s.no_user_kernel : s.no_builtin_kernel);
  int W = 0, E = 0;
  rc = s.mapping == kUpToFourPerLane ? first_order_mapping(s, desc, W, E) : one_per_lane_mapping(s, desc, W, E);
  if (rc != MI355_OK) return rc;
  DeviceConfig dc;
  rc = configure(dc);
  if (rc != MI355_OK) return rc;
  if (io.B == 0) return MI355_OK;
  if (!io.x0 || !io.x_out || !io.f_out) return fail(MI355_ERR_INVALID_ARGUMENT, "null x0 / x_out / f_out");
  hipStream_t stream = static_cast<hipStream_t>(io.stream);
  MI355_ENTER_DEVICE(ctx);
  rc = upload_params(ctx, &desc, W, E, stream);
  if (rc != MI355_OK) return rc;
  SolveArgs args = solver_args(ctx, desc, io);
  rc = setup_trace(ctx, &desc, io.B, stream, args);
  if (rc != MI355_OK) return rc;
  return dispatch(W, E, desc.objective, args, dc, stream);
}

// a caller's config, or the defaults
template <class Config>
Config config_or_default(const Config* config, int (*defaults)(Config*)) {
  Config c;
  defaults(&c);
  return config ? *config : c;
}

int first_order_minimize_batch(const char* name, int method, mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc,
                               const mi355_armijo_config* config, const Batch& io) {
  const Solver s = first_order_solver(name);
  return minimize_batch<FirstOrderDeviceConfig>(
      s, ctx, desc, io,
      [&](FirstOrderDeviceConfig& dc) -> int {
        const mi355_armijo_config c = config_or_default(config, &mi355_armijo_default_config);
        // (the search must end: alpha shrinks towards alpha_min)
        if (!(c.rho > 0.0 && c.rho < 1.0) || !(c.alpha_min > 0.0))
          return refuse(MI355_ERR_INVALID_ARGUMENT, s, ": the Armijo config needs 0 < rho < 1 and alpha_min > 0");
        dc.armijo_c = c.c;
        dc.armijo_rho = c.rho;
        dc.armijo_alpha_min = c.alpha_min;
        // measurement switch (scripts/first_order_bench.py): 1 = the Armijo trials run eval instead of value()
        dc.eval_trials = ctx->debug_cg_eval_trials ? 1 : 0;
        return MI355_OK;
      },
      [&](int W, int E, int objective, const SolveArgs& args, const FirstOrderDeviceConfig& dc, hipStream_t stream) {
        return dispatch_first_order(ctx, method, W, E, objective, args, dc, stream);
      });
}

}  // namespace

extern "C" {

// ---- TrustRegionNewton (trust_region_kernel.hpp) -------------------------------------------------------------------
int mi355_trust_region_default_config(mi355_trust_region_config* out) {
  if (!out) return fail(MI355_ERR_INVALID_ARGUMENT, "null config");
  out->initial_radius = 1.0;        // trust_region_newton.h TrustRegionNewtonConfig defaults
  out->max_radius = 1e10;
  out->acceptance_threshold = 0.15;
  out->shrink_factor = 0.25;
  out->expand_factor = 2.0;
  out->rho_low = 0.25;
  out->rho_high = 0.75;
  out->cg_forcing_coefficient = 0.5;
  out->cg_max_iterations_floor = 10;
  out->min_radius = 1e-12;
  out->rejection_retry_limit = 50;
  return MI355_OK;
}

int mi355_trust_region_newton_minimize_batch(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc,
                                             const mi355_trust_region_config* config, int64_t B, const double* x0,
                                             double* x_out, double* f_out, double* g_out,
                                             mi355_lbfgs_progress* progress_out, void* stream) {
  return minimize_batch<TrustRegionDeviceConfig>(
      kTrustRegionNewton, ctx, desc, {B, x0, x_out, f_out, g_out, progress_out, stream},
      [&](TrustRegionDeviceConfig& dc) -> int {
        const mi355_trust_region_config c = config_or_default(config, &mi355_trust_region_default_config);
        dc.initial_radius = c.initial_radius;
        dc.max_radius = c.max_radius;
        dc.acceptance_threshold = c.acceptance_threshold;
        dc.shrink_factor = c.shrink_factor;
        dc.expand_factor = c.expand_factor;
        dc.rho_low = c.rho_low;
        dc.rho_high = c.rho_high;
        dc.cg_forcing_coefficient = c.cg_forcing_coefficient;
        dc.min_radius = c.min_radius;
        dc.cg_extra_iterations = c.cg_max_iterations_floor > 0 ? c.cg_max_iterations_floor : 0;
        dc.rejection_retry_limit =
            c.rejection_retry_limit < 0 ? 0 : (c.rejection_retry_limit > 1000 ? 1000 : c.rejection_retry_limit);
        return MI355_OK;
      },
      [&](int W, int, int objective, const SolveArgs& args, const TrustRegionDeviceConfig& dc, hipStream_t s) {
        return dispatch_trust_region(ctx, W, objective, args, dc, s);
      });
}

// ---- NelderMead (nelder_mead_kernel.hpp) ---------------------------------------------------------------------------
int mi355_nelder_mead_default_config(mi355_nelder_mead_config* out) {
  if (!out) return fail(MI355_ERR_INVALID_ARGUMENT, "null config");
  out->rho = 1.0;             // nelder_mead.h:58-64
  out->xi = 20.0;
  out->gamma = 0.1;
  out->sigma = 0.5;
  out->degenerate_tol = 1e-8;
  out->mode = MI355_NM_MODE_VALUE;
  return MI355_OK;
}

int mi355_nelder_mead_minimize_batch(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc,
                                     const mi355_nelder_mead_config* config, int64_t B, const double* x0, double* x_out,
                                     double* f_out, double* g_out, mi355_lbfgs_progress* progress_out, void* stream) {
  return minimize_batch<NelderMeadDeviceConfig>(
      kNelderMead, ctx, desc, {B, x0, x_out, f_out, g_out, progress_out, stream},
      [&](NelderMeadDeviceConfig& dc) -> int {
        const mi355_nelder_mead_config c = config_or_default(config, &mi355_nelder_mead_default_config);
        if (c.mode != MI355_NM_MODE_VALUE && c.mode != MI355_NM_MODE_FIRST)
          return refuse(MI355_ERR_INVALID_ARGUMENT, kNelderMead, ": mode must be MI355_NM_MODE_VALUE or MI355_NM_MODE_FIRST");
        dc.rho = c.rho;
        dc.xi = c.xi;
        dc.gamma = c.gamma;
        dc.sigma = c.sigma;
        dc.degenerate_tol = c.degenerate_tol;
        dc.first_mode = c.mode == MI355_NM_MODE_FIRST ? 1 : 0;
        return MI355_OK;
      },
      [&](int W, int, int objective, const SolveArgs& args, const NelderMeadDeviceConfig& dc, hipStream_t s) {
        return dispatch_nelder_mead(ctx, W, objective, args, dc, s);
      });
}

// ---- NewtonDescent (newton_descent_kernel.hpp) ---------------------------------------------------------------------
int mi355_newton_descent_default_config(mi355_newton_descent_config* out) {
  if (!out) return fail(MI355_ERR_INVALID_ARGUMENT, "null config");
  out->safe_guard = 1e-5;   // newton_descent.h:69
  out->armijo_c = 0.2;      // linesearch/armijo.h:85-86
  out->armijo_rho = 0.9;
  return MI355_OK;
}

int mi355_newton_descent_minimize_batch(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc,
                                        const mi355_newton_descent_config* config, int64_t B, const double* x0,
                                        double* x_out, double* f_out, double* g_out, mi355_lbfgs_progress* progress_out,
                                        void* stream) {
  return minimize_batch<NewtonDescentDeviceConfig>(
      kNewtonDescent, ctx, desc, {B, x0, x_out, f_out, g_out, progress_out, stream},
      [&](NewtonDescentDeviceConfig& dc) -> int {
        const mi355_newton_descent_config c = config_or_default(config, &mi355_newton_descent_default_config);
        dc.safe_guard = c.safe_guard;
        dc.armijo_c = c.armijo_c;
        dc.armijo_rho = c.armijo_rho;
        return MI355_OK;
      },
      [&](int W, int, int objective, const SolveArgs& args, const NewtonDescentDeviceConfig& dc, hipStream_t s) {
        return dispatch_newton_descent(ctx, W, objective, args, dc, s);
      });
}

// ---- GradientDescent / ConjugatedGradientDescent (first_order_kernel.hpp) -------------------------------------------
int mi355_armijo_default_config(mi355_armijo_config* out) {
  if (!out) return fail(MI355_ERR_INVALID_ARGUMENT, "null config");
  out->c = 0.2;            // linesearch/armijo.h:49-50
  out->rho = 0.9;
  out->alpha_min = 1e-8;   // :56
  return MI355_OK;
}

int mi355_gradient_descent_minimize_batch(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const double* x0,
                                          double* x_out, double* f_out, double* g_out,
                                          mi355_lbfgs_progress* progress_out, void* stream) {
  return first_order_minimize_batch("GradientDescent", kGradientDescent, ctx, desc, nullptr,
                                    {B, x0, x_out, f_out, g_out, progress_out, stream});
}

int mi355_conjugated_gradient_descent_minimize_batch(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc,
                                                     const mi355_armijo_config* config, int64_t B, const double* x0,
                                                     double* x_out, double* f_out, double* g_out,
                                                     mi355_lbfgs_progress* progress_out, void* stream) {
  return first_order_minimize_batch("ConjugatedGradientDescent", kConjugatedGradientDescent, ctx, desc, config,
                                    {B, x0, x_out, f_out, g_out, progress_out, stream});
}

}  // extern "C"

// ---- Lbfgs<F, m, MoreThuente> with ScalarType = float (lbfgs_f32_kernel.hpp) ------------------------------------------
// Opt-in: the fp64 entry points are untouched and a float function that does not ask for this path is still widened.
namespace {

int f32_refuse(const char* text) { return fail(MI355_ERR_UNSUPPORTED, std::string("Lbfgs float32") + text); }

// Everything the float entry points check before the device is touched: the refusals (MI355_ERR_UNSUPPORTED, with the
// reason), validate()'s argument checks, the lane mapping.
int f32_check(const mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, int& W, int& E) {
  if (!desc) return fail(MI355_ERR_INVALID_ARGUMENT, "null desc");
  if (desc->objective != MI355_OBJ_ROSENBROCK && desc->objective != MI355_OBJ_DIAG_QUADRATIC)
    return f32_refuse(" is built for the Rosenbrock and DiagQuadratic objectives (no user functors, ridge forms or composites)");
  if (desc->n > MI355_LBFGS_MAX_N) return f32_refuse(" is built for n <= 256");
  if (desc->per_problem_data != nullptr) return f32_refuse(" takes no per-problem data");
  const int rc = validate(ctx, desc, B);
  if (rc != MI355_OK) return rc;
  if (desc->linesearch != MI355_LS_MORE_THUENTE) return f32_refuse(" is built with the More-Thuente line search only");
  if (desc->arithmetic == MI355_ARITH_FMA) return f32_refuse(" is built for the exact arithmetic only (no MI355_ARITH_FMA)");
  if (desc->history_placement == MI355_HISTORY_Y_IN_REGISTERS)
    return f32_refuse(" keeps both halves of the history in LDS (no MI355_HISTORY_Y_IN_REGISTERS)");
  if (desc->hessian_from_functor || desc->hessian_diagonal != nullptr || desc->hessian_condition_stop > 0.0)
    return f32_refuse(" is built for First-mode functions (no hessian_from_functor, hessian_diagonal or hessian_condition_stop)");
  if (desc->trace != nullptr) return f32_refuse(" records no per-iteration trace");
  W = desc->lanes_per_problem;
  E = desc->elems_per_lane;
  if (W == 0 && E == 0) {
    W = 8;
    while (W < desc->n && W < 64) W <<= 1;
  }
  if (E == 0 && (W == 8 || W == 16 || W == 32 || W == 64)) E = (desc->n <= W) ? 1 : ((desc->n <= 2 * W) ? 2 : 4);
  const bool built = ((W == 8 || W == 16 || W == 32 || W == 64) && E == 1) || (W == 64 && (E == 2 || E == 4));
  if (!built || W * E < desc->n)
    return f32_refuse(": the mapping must cover n with 8, 16, 32 or 64 lanes at one coordinate per lane, or 64 lanes at "
                      "two or four");
  return MI355_OK;
}

// the objective's parameters as floats (each double converted once), through the context's parameter blob
int f32_upload_params(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int W, int E, hipStream_t stream) {
  if (desc->n_params == 0) return MI355_OK;
  std::vector<float> as_float(static_cast<size_t>(desc->n_params) + 1, 0.0f);   // (+ 1: room to round up to whole doubles)
  for (int i = 0; i < desc->n_params; ++i) as_float[i] = static_cast<float>(desc->objective_params[i]);
  std::vector<double>& h = ctx->params_host;
  h.assign((static_cast<size_t>(desc->n_params) + 1) / 2, 0.0);
  std::memcpy(h.data(), as_float.data(), h.size() * sizeof(double));
  mi355_lbfgs_desc blob = *desc;
  blob.objective_params = h.data();
  blob.n_params = static_cast<int>(h.size());
  return upload_params(ctx, &blob, W, E, stream);
}

}  // namespace

extern "C" int mi355_lbfgs_minimize_batch_f32(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const float* x0,
                                              float* x_out, float* f_out, float* g_out,
                                              mi355_lbfgs_progress* progress_out, void* stream_) {
  int W = 0, E = 0;
  int rc = f32_check(ctx, desc, B, W, E);
  if (rc != MI355_OK) return rc;
  if (B == 0) return MI355_OK;
  if (!x0 || !x_out || !f_out) return fail(MI355_ERR_INVALID_ARGUMENT, "null x0 / x_out / f_out");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(ctx);
  rc = f32_upload_params(ctx, desc, W, E, stream);
  if (rc != MI355_OK) return rc;
  SolveArgs args;
  std::memset(&args, 0, sizeof(args));
  args.progress_out = progress_out;
  args.B = B;
  args.n = desc->n;
  args.m = desc->m;
  args.stop = desc->stop;
  f32::LbfgsF32Args fa;
  fa.x0 = x0;
  fa.x_out = x_out;
  fa.f_out = f_out;
  fa.g_out = g_out;
  fa.obj_params = reinterpret_cast<const float*>(ctx->params_dev);
  fa.stop_x_delta = static_cast<float>(desc->stop.x_delta);
  fa.stop_f_delta = static_cast<float>(desc->stop.f_delta);
  fa.stop_gradient_norm = static_cast<float>(desc->stop.gradient_norm);
  fa.stop_past_delta = static_cast<float>(desc->stop.past_delta);
  return dispatch_lbfgs_f32(ctx, W, E, desc->objective, args, fa, stream);
}

extern "C" int mi355_lbfgs_eval_batch_f32(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const float* x,
                                          float* f_out, float* g_out, void* stream_) {
  int W = 0, E = 0;
  int rc = f32_check(ctx, desc, B, W, E);
  if (rc != MI355_OK) return rc;
  if (B == 0) return MI355_OK;
  if (!x || !f_out) return fail(MI355_ERR_INVALID_ARGUMENT, "null x / f_out");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(ctx);
  rc = f32_upload_params(ctx, desc, W, E, stream);
  if (rc != MI355_OK) return rc;
  return dispatch_eval_f32(W, E, desc->objective, x, f_out, g_out, reinterpret_cast<const float*>(ctx->params_dev), B,
                           desc->n, stream);
}
