// ask_tell_entry.hip — the C entry points of the four ask/tell (reverse communication) paths (include/mi355_lbfgs.h):
// mi355_lbfgs_ask_tell_* (Lbfgs in double), mi355_lbfgs_ask_tell_f32_* (Lbfgs in float), mi355_lbfgsb_ask_tell_*
// (Lbfgsb) and mi355_lbfgs_ask_tell_wide_* (Lbfgs in double above n = 256, a workgroup per problem).  Each path is its traits, its handle struct, its own refusals and its C functions; the rest —
// the shared refusals, the one device allocation and its layout, the bodies of the entry points — is ask_tell_host.hpp.
// The kernels are behind dispatch_lbfgs_ask_tell.hip, dispatch_lbfgs_ask_tell_f32.hip, dispatch_lbfgsb_ask_tell.hip and
// dispatch_lbfgs_ask_tell_wide.hip, those of a compacted handle (mi355_ask_tell_compact_*) behind their *_listed.hip
// twins and dispatch_ask_tell_compact.hip (the wide path's compaction: its listed unit).
#include "ask_tell_host.hpp"
#include "lbfgs_ask_tell_config.hpp"
#include "lbfgs_ask_tell_f32_config.hpp"
#include "lbfgsb_ask_tell_config.hpp"
#include "lbfgs_ask_tell_wide_config.hpp"

using namespace mi355;
namespace host = mi355::ask_tell_host;

namespace mi355 {
namespace ask_tell_host {

struct LbfgsPath {
  using Scalar = double;
  using Scalars = ask_tell::Scalars;
  using Args = ask_tell::Args;
  using ResultArgs = ask_tell::ResultArgs;
  static long long row(int m, int P) { return ask_tell::row_doubles(m, P); }
  static constexpr auto step = &dispatch_ask_tell_step;
  static constexpr auto listed_step = &dispatch_ask_tell_listed_step;
  static constexpr int kFinished = ask_tell::kPhaseFinished;
  static constexpr auto results = &dispatch_ask_tell_results;
  static constexpr const char* kPrefix = "Lbfgs ask/tell";
  static constexpr const char* kWhat = "ask/tell";
  static constexpr bool kRefusesLargeM = false;  // validate() words the m limit
};

struct LbfgsF32Path {
  using Scalar = float;
  using Scalars = ask_tell_f32::Scalars;
  using Args = ask_tell_f32::Args;
  using ResultArgs = ask_tell_f32::ResultArgs;
  static long long row(int m, int P) { return ask_tell_f32::row_floats(m, P); }
  static constexpr auto step = &dispatch_ask_tell_f32_step;
  static constexpr auto listed_step = &dispatch_ask_tell_f32_listed_step;
  static constexpr int kFinished = ask_tell_f32::kPhaseFinished;
  static constexpr auto results = &dispatch_ask_tell_f32_results;
  static constexpr const char* kPrefix = "Lbfgs ask/tell f32";
  static constexpr const char* kWhat = "ask/tell f32";
  static constexpr bool kRefusesLargeM = true;
};

struct LbfgsbPath {
  using Scalar = double;
  using Scalars = ask_tell_box::Scalars;
  using Args = ask_tell_box::Args;
  using ResultArgs = ask_tell_box::ResultArgs;
  static long long row(int m, int P) { return ask_tell_box::row_doubles(m, ask_tell_box_capacity(m), P); }
  static int step(mi355_lbfgs_ctx* ctx, int, int E, const Args& a, hipStream_t stream) {  // (W is kLanes)
    return dispatch_ask_tell_box_step(ctx, E, a, stream);
  }
  static int listed_step(mi355_lbfgs_ctx* ctx, int, int E, const Args& a, const long long* ids, long long listed,
                         hipStream_t stream) {
    return dispatch_ask_tell_box_listed_step(ctx, E, a, ids, listed, stream);
  }
  static constexpr int kFinished = ask_tell_box::kPhaseFinished;
  static constexpr auto results = &dispatch_ask_tell_box_results;
  static constexpr const char* kPrefix = "Lbfgsb ask/tell";
  static constexpr const char* kWhat = "ask/tell";
};

// Above n = 256: a workgroup per problem.  The handle's (W, E) hold the padded vector length np at one "coordinate":
// W * E is what row() and the result gather take as the width of a state vector.
struct LbfgsWidePath {
  using Scalar = double;
  using Scalars = ask_tell_wide::Scalars;
  using Args = ask_tell_wide::Args;
  using ResultArgs = ask_tell_wide::ResultArgs;
  static long long row(int m, int P) { return ask_tell_wide::row_doubles(m, P); }
  static int step(mi355_lbfgs_ctx* ctx, int, int, const Args& a, hipStream_t stream) {
    return dispatch_ask_tell_wide_step(ctx, a, stream);
  }
  static int listed_step(mi355_lbfgs_ctx* ctx, int, int, const Args& a, const long long* ids, long long listed,
                         hipStream_t stream) {
    return dispatch_ask_tell_wide_listed_step(ctx, a, ids, listed, stream);
  }
  static constexpr int kFinished = ask_tell_wide::kPhaseFinished;
  static constexpr auto results = &dispatch_ask_tell_wide_results;
  static constexpr const char* kPrefix = "Lbfgs ask/tell wide";
  static constexpr const char* kWhat = "ask/tell wide";
};

}  // namespace ask_tell_host

// (defined in dispatch_lbfgs_ask_tell_wide_listed.hip)
template <>
int dispatch_ask_tell_compact<double, ask_tell_wide::Scalars, ask_tell_wide::kPhaseFinished>(
    const ask_tell_compact::Args<double, ask_tell_wide::Scalars>& args, hipStream_t stream);

}  // namespace mi355

struct mi355_lbfgs_ask_tell : host::Handle<host::LbfgsPath> {};

struct mi355_lbfgs_ask_tell_f32 : host::Handle<host::LbfgsF32Path> {
  // static_cast<float> of the stop record's thresholds, converted once per call
  void finish_args(ask_tell_f32::Args& a) const {
    a.stop_x_delta = static_cast<float>(stop.x_delta);
    a.stop_f_delta = static_cast<float>(stop.f_delta);
    a.stop_gradient_norm = static_cast<float>(stop.gradient_norm);
    a.stop_past_delta = static_cast<float>(stop.past_delta);
  }
};

// extras: the handle's copy of the box, lower then upper (n each, or B n each); counters: active, asks[5], the NaN flag
struct mi355_lbfgsb_ask_tell : host::Handle<host::LbfgsbPath> {
  double* lower = nullptr;
  double* upper = nullptr;
  unsigned long long* asks = nullptr;
  int* nan_flag = nullptr;
  long long box_stride = 0;  // of the handle's copy: 0 (one box) or n
  static constexpr int kCounterWords = 1 + ask_tell_box::kAskKinds + 1;
  size_t box_doubles() const { return static_cast<size_t>(n) * ((box_stride != 0) ? static_cast<size_t>(B) : 1); }
  size_t extra_bytes() const { return 2 * box_doubles() * sizeof(double); }
  void place_extras(char* extras) {
    lower = reinterpret_cast<double*>(extras);
    upper = lower + box_doubles();
    asks = active + 1;
    nan_flag = reinterpret_cast<int*>(asks + ask_tell_box::kAskKinds);
  }
  void finish_args(ask_tell_box::Args& a) const {
    a.lower = lower;
    a.upper = upper;
    a.box_stride = box_stride;
    a.asks = asks;
  }
};

struct mi355_lbfgs_ask_tell_wide : host::Handle<host::LbfgsWidePath> {
  void finish_args(ask_tell_wide::Args& a) const { a.d_in_lds = 0; }  // (the launch decides)
};

namespace {

// The wide path's refusals around the shared ones, everything before the device is touched
int check_wide(const mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B) {
  using T = host::LbfgsWidePath;
  return host::check_common<T>(
      ctx, desc, B,
      [&] {
        if (desc->n <= MI355_LBFGS_MAX_N)
          return host::refuse<T>(" is built for n > 256: mi355_lbfgs_ask_tell_create takes n <= 256");
        if (desc->arithmetic == MI355_ARITH_FMA)
          return host::refuse<T>(" is built for the exact arithmetic only (no MI355_ARITH_FMA)");
        if (desc->history_placement == MI355_HISTORY_Y_IN_REGISTERS)
          return host::refuse<T>(" keeps the history in device memory between calls (no MI355_HISTORY_Y_IN_REGISTERS)");
        if (desc->hessian_from_functor) return host::refuse<T>(" is built for First-mode functions (no hessian_from_functor)");
        if (desc->hessian_diagonal != nullptr) return host::refuse<T>(" is built for First-mode functions (no hessian_diagonal)");
        if (desc->hessian_condition_stop > 0.0)
          return host::refuse<T>(" is built for First-mode functions (no hessian_condition_stop)");
        return static_cast<int>(MI355_OK);
      },
      [&] {
        if (desc->lanes_per_problem != 0 || desc->elems_per_lane != 0)
          return host::refuse<T>(" chooses its own mapping, a workgroup per problem: leave lanes_per_problem and elems_per_lane 0");
        return static_cast<int>(MI355_OK);
      },
      /*allow_wide=*/true);
}

// Lbfgsb's own refusals around the shared ones, then the box arguments
int check_box(const mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const double* lower,
              const double* upper, int64_t box_stride) {
  using T = host::LbfgsbPath;
  const int rc = host::check_common<T>(
      ctx, desc, B,
      [&] {
        if (desc->arithmetic == MI355_ARITH_FMA)
          return host::refuse<T>(" is built for the reference-order arithmetic only (no MI355_ARITH_FMA: the relaxed algebra has "
                                 "no ask/tell form)");
        if (desc->m > 8) return host::refuse<T>(" is built for m <= 8 (m = 9, 10 take 32 lanes per problem)");
        if (desc->n > 64) return host::refuse<T>(" is built for n <= 64");
        return static_cast<int>(MI355_OK);
      },
      [&] {
        if (desc->hessian_from_functor) return host::refuse<T>(": Lbfgsb has no preconditioned path (no hessian_from_functor)");
        if (desc->hessian_diagonal != nullptr) return host::refuse<T>(": Lbfgsb has no preconditioned path (no hessian_diagonal)");
        if (desc->hessian_condition_stop > 0.0) return host::refuse<T>(" computes no Hessian (no hessian_condition_stop)");
        if (desc->lanes_per_problem != 0 || desc->elems_per_lane != 0 || desc->history_placement != 0)
          return host::refuse<T>(" chooses its own mapping: leave lanes_per_problem, elems_per_lane and history_placement 0");
        return static_cast<int>(MI355_OK);
      });
  if (rc != MI355_OK) return rc;
  if ((lower == nullptr) != (upper == nullptr))
    return fail(MI355_ERR_INVALID_ARGUMENT, "lower and upper must both be given or both be NULL");
  if (box_stride != 0 && !lower)
    return fail(MI355_ERR_INVALID_ARGUMENT, "per-problem bounds: lower and upper are required");
  if (box_stride != 0 && box_stride < desc->n)
    return fail(MI355_ERR_INVALID_ARGUMENT, "per-problem bounds: box_stride must be >= n (0: one shared box)");
  return MI355_OK;
}

// x0 into the state, the caller's box (or the reference's default one) into the handle's copy.  A NaN bound makes the
// breakpoint order of the Cauchy search undefined in the reference as well (the check of
// mi355_lbfgsb_minimize_batch_host, taken on the handle's copy: the caller's arrays are device memory here).
int init_box(mi355_lbfgsb_ask_tell& h, const double* x0, const double* lower, const double* upper, int64_t box_stride,
             long long row, hipStream_t stream) {
  ask_tell_box::InitArgs ia;
  ia.vectors = h.vectors;
  ia.scalars = h.scalars;
  ia.x_eval = h.x_eval;
  ia.x0 = x0;
  ia.lower = h.lower;
  ia.upper = h.upper;
  ia.lower_in = lower;
  ia.upper_in = upper;
  ia.box_stride_in = box_stride;
  ia.asks = h.asks;
  ia.nan_flag = h.nan_flag;
  ia.B = h.B;
  ia.row = row;
  ia.n = h.n;
  const int rc = dispatch_ask_tell_box_init(ia, stream);
  if (rc != MI355_OK || lower == nullptr) return rc;
  int flag = 0;
  hipError_t he = hipMemcpyAsync(&flag, h.nan_flag, sizeof(flag), hipMemcpyDeviceToHost, stream);
  if (he == hipSuccess) he = hipStreamSynchronize(stream);
  if (he != hipSuccess) return fail(MI355_ERR_HIP, std::string("ask/tell box check: ") + hipGetErrorString(he));
  if (flag != 0) return fail(MI355_ERR_INVALID_ARGUMENT, "NaN bound");
  return MI355_OK;
}

}  // namespace

extern "C" {

// ---- Lbfgs in double --------------------------------------------------------------------------------------------------
int mi355_lbfgs_ask_tell_create(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const double* x0,
                                void* stream, mi355_lbfgs_ask_tell** out) {
  return host::create(
      ctx, desc, B, x0, stream, out,
      [&](mi355_lbfgs_ask_tell& h) { return host::check_lbfgs<host::LbfgsPath>(ctx, desc, B, h.W, h.E); },
      [&](mi355_lbfgs_ask_tell& h, long long row, hipStream_t s) {
        return dispatch_ask_tell_init(host::step_args(&h, nullptr, nullptr), x0, row, s);
      });
}
int mi355_lbfgs_ask_tell_x(mi355_lbfgs_ask_tell* handle, const double** x_eval) { return host::x(handle, x_eval); }
int mi355_lbfgs_ask_tell_step(mi355_lbfgs_ask_tell* handle, const double* f, const double* g, int64_t* active_host,
                              void* stream) {
  return host::step(handle, f, g, active_host, stream);
}
int mi355_lbfgs_ask_tell_active(mi355_lbfgs_ask_tell* handle, const int64_t** active_dev) {
  return host::active(handle, active_dev);
}
int mi355_lbfgs_ask_tell_results(mi355_lbfgs_ask_tell* handle, double* x_out, double* f_out, double* g_out,
                                 mi355_lbfgs_progress* progress_out, void* stream) {
  return host::results(handle, x_out, f_out, g_out, progress_out, stream);
}
int mi355_lbfgs_ask_tell_destroy(mi355_lbfgs_ask_tell* handle) { return host::destroy(handle); }

// ---- Lbfgs in double above n = 256 ------------------------------------------------------------------------------------
int mi355_lbfgs_ask_tell_wide_create(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const double* x0,
                                     void* stream, mi355_lbfgs_ask_tell_wide** out) {
  return host::create(
      ctx, desc, B, x0, stream, out,
      [&](mi355_lbfgs_ask_tell_wide& h) {
        const int rc = check_wide(ctx, desc, B);
        if (rc != MI355_OK) return rc;
        h.W = static_cast<int>(ask_tell_wide::padded(desc->n));
        h.E = 1;
        return static_cast<int>(MI355_OK);
      },
      [&](mi355_lbfgs_ask_tell_wide& h, long long row, hipStream_t s) {
        return dispatch_ask_tell_wide_init(host::step_args(&h, nullptr, nullptr), x0, row, s);
      });
}
int mi355_lbfgs_ask_tell_wide_x(mi355_lbfgs_ask_tell_wide* handle, const double** x_eval) { return host::x(handle, x_eval); }
int mi355_lbfgs_ask_tell_wide_step(mi355_lbfgs_ask_tell_wide* handle, const double* f, const double* g,
                                   int64_t* active_host, void* stream) {
  return host::step(handle, f, g, active_host, stream);
}
int mi355_lbfgs_ask_tell_wide_active(mi355_lbfgs_ask_tell_wide* handle, const int64_t** active_dev) {
  return host::active(handle, active_dev);
}
int mi355_lbfgs_ask_tell_wide_results(mi355_lbfgs_ask_tell_wide* handle, double* x_out, double* f_out, double* g_out,
                                      mi355_lbfgs_progress* progress_out, void* stream) {
  return host::results(handle, x_out, f_out, g_out, progress_out, stream);
}
int mi355_lbfgs_ask_tell_wide_destroy(mi355_lbfgs_ask_tell_wide* handle) { return host::destroy(handle); }

// ---- Lbfgs in float ---------------------------------------------------------------------------------------------------
int mi355_lbfgs_ask_tell_f32_create(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const float* x0,
                                    void* stream, mi355_lbfgs_ask_tell_f32** out) {
  return host::create(
      ctx, desc, B, x0, stream, out,
      [&](mi355_lbfgs_ask_tell_f32& h) { return host::check_lbfgs<host::LbfgsF32Path>(ctx, desc, B, h.W, h.E); },
      [&](mi355_lbfgs_ask_tell_f32& h, long long row, hipStream_t s) {
        return dispatch_ask_tell_f32_init(host::step_args(&h, nullptr, nullptr), x0, row, s);
      });
}
int mi355_lbfgs_ask_tell_f32_x(mi355_lbfgs_ask_tell_f32* handle, const float** x_eval) { return host::x(handle, x_eval); }
int mi355_lbfgs_ask_tell_f32_step(mi355_lbfgs_ask_tell_f32* handle, const float* f, const float* g,
                                  int64_t* active_host, void* stream) {
  return host::step(handle, f, g, active_host, stream);
}
int mi355_lbfgs_ask_tell_f32_active(mi355_lbfgs_ask_tell_f32* handle, const int64_t** active_dev) {
  return host::active(handle, active_dev);
}
int mi355_lbfgs_ask_tell_f32_results(mi355_lbfgs_ask_tell_f32* handle, float* x_out, float* f_out, float* g_out,
                                     mi355_lbfgs_progress* progress_out, void* stream) {
  return host::results(handle, x_out, f_out, g_out, progress_out, stream);
}
int mi355_lbfgs_ask_tell_f32_destroy(mi355_lbfgs_ask_tell_f32* handle) { return host::destroy(handle); }

// ---- Lbfgsb -----------------------------------------------------------------------------------------------------------
int mi355_lbfgsb_ask_tell_create(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, const double* lower,
                                 const double* upper, int64_t box_stride, int64_t B, const double* x0, void* stream,
                                 mi355_lbfgsb_ask_tell** out) {
  return host::create(
      ctx, desc, B, x0, stream, out,
      [&](mi355_lbfgsb_ask_tell& h) {
        const int rc = check_box(ctx, desc, B, lower, upper, box_stride);
        if (rc != MI355_OK) return rc;
        h.W = ask_tell_box::kLanes;
        h.E = (desc->n <= 16) ? 1 : ((desc->n <= 32) ? 2 : 4);
        h.box_stride = (box_stride != 0) ? desc->n : 0;
        return static_cast<int>(MI355_OK);
      },
      [&](mi355_lbfgsb_ask_tell& h, long long row, hipStream_t s) {
        return init_box(h, x0, lower, upper, box_stride, row, s);
      });
}
int mi355_lbfgsb_ask_tell_x(mi355_lbfgsb_ask_tell* handle, const double** x_eval) { return host::x(handle, x_eval); }
int mi355_lbfgsb_ask_tell_step(mi355_lbfgsb_ask_tell* handle, const double* f, const double* g, int64_t* active_host,
                               void* stream) {
  return host::step(handle, f, g, active_host, stream);
}
int mi355_lbfgsb_ask_tell_active(mi355_lbfgsb_ask_tell* handle, const int64_t** active_dev) {
  return host::active(handle, active_dev);
}
int mi355_lbfgsb_ask_tell_asks(mi355_lbfgsb_ask_tell* handle, int64_t* counts_host, void* stream_) {
  if (!handle || !counts_host) return fail(MI355_ERR_INVALID_ARGUMENT, "null argument");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(handle->ctx);
  unsigned long long counts[ask_tell_box::kAskKinds];
  HIP_TRY(hipMemcpyAsync(counts, handle->asks, sizeof(counts), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int i = 0; i < ask_tell_box::kAskKinds; ++i) counts_host[i] = static_cast<int64_t>(counts[i]);
  return MI355_OK;
}
int mi355_lbfgsb_ask_tell_results(mi355_lbfgsb_ask_tell* handle, double* x_out, double* f_out, double* g_out,
                                  mi355_lbfgs_progress* progress_out, void* stream) {
  return host::results(handle, x_out, f_out, g_out, progress_out, stream);
}
int mi355_lbfgsb_ask_tell_destroy(mi355_lbfgsb_ask_tell* handle) { return host::destroy(handle); }

// ---- the list of the live problems, for the four handle types ----------------------------------------------------------
int mi355_ask_tell_compact_lbfgs(mi355_lbfgs_ask_tell* handle, int64_t* listed_host, void* stream) {
  return host::compact(handle, listed_host, stream);
}
int mi355_ask_tell_compact_lbfgs_f32(mi355_lbfgs_ask_tell_f32* handle, int64_t* listed_host, void* stream) {
  return host::compact(handle, listed_host, stream);
}
int mi355_ask_tell_compact_lbfgsb(mi355_lbfgsb_ask_tell* handle, int64_t* listed_host, void* stream) {
  return host::compact(handle, listed_host, stream);
}
int mi355_lbfgs_ask_tell_wide_compact(mi355_lbfgs_ask_tell_wide* handle, int64_t* listed_host, void* stream) {
  return host::compact(handle, listed_host, stream);
}
int mi355_lbfgs_ask_tell_wide_ids(mi355_lbfgs_ask_tell_wide* handle, const int64_t** ids_dev, int64_t* listed) {
  return host::ids(handle, ids_dev, listed);
}
int mi355_ask_tell_ids_lbfgs(mi355_lbfgs_ask_tell* handle, const int64_t** ids_dev, int64_t* listed) {
  return host::ids(handle, ids_dev, listed);
}
int mi355_ask_tell_ids_lbfgs_f32(mi355_lbfgs_ask_tell_f32* handle, const int64_t** ids_dev, int64_t* listed) {
  return host::ids(handle, ids_dev, listed);
}
int mi355_ask_tell_ids_lbfgsb(mi355_lbfgsb_ask_tell* handle, const int64_t** ids_dev, int64_t* listed) {
  return host::ids(handle, ids_dev, listed);
}

}  // extern "C"
