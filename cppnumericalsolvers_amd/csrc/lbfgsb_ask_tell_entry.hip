// lbfgsb_ask_tell_entry.hip — the C entry points of the ask/tell (reverse communication) L-BFGS-B (include/mi355_lbfgs.h,
// mi355_lbfgsb_ask_tell_*): the refusals, the solve handle with its one device allocation (state, evaluation buffer, the
// handle's copy of the box, counters), and the calls into dispatch_lbfgsb_ask_tell.hip.  No kernel lives here.
#include <new>

#include "engine_internal.hpp"
#include "lbfgsb_ask_tell_config.hpp"

using namespace mi355;

// One solve in flight: the state of all B problems in ONE device allocation
//   [ x_eval B n | vectors B row | scalars B | lower, upper (n each, or B n each) | active | asks[5] | NaN flag ]
struct mi355_lbfgsb_ask_tell {
  mi355_lbfgs_ctx* ctx = nullptr;
  char* block = nullptr;
  size_t bytes = 0;
  double* x_eval = nullptr;
  double* vectors = nullptr;
  ask_tell_box::Scalars* scalars = nullptr;
  double* lower = nullptr;
  double* upper = nullptr;
  unsigned long long* active = nullptr;
  unsigned long long* asks = nullptr;
  int* nan_flag = nullptr;
  int64_t B = 0;
  long long box_stride = 0;  // of the handle's copy: 0 (one box) or n
  int n = 0, m = 0, E = 0, M = 0;
  mi355_lbfgs_stop stop;
};

namespace {

int refuse(const char* text) { return fail(MI355_ERR_UNSUPPORTED, std::string("Lbfgsb ask/tell") + text); }

// Everything checked before the device is touched: the refusals (MI355_ERR_UNSUPPORTED, with the reason), then
// validate()'s argument checks on the fields this path reads (the objective and its parameters are not among them: the
// caller evaluates).
int check(const mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B) {
  if (!ctx) return fail(MI355_ERR_INVALID_ARGUMENT, "null context");
  if (!desc) return fail(MI355_ERR_INVALID_ARGUMENT, "null desc");
  if (desc->linesearch == MI355_LS_HAGER_ZHANG)
    return refuse(" is built with the More-Thuente line search only (no Hager-Zhang)");
  if (desc->arithmetic == MI355_ARITH_FMA)
    return refuse(" is built for the reference-order arithmetic only (no MI355_ARITH_FMA: the relaxed algebra has no ask/tell form)");
  if (desc->m > 8) return refuse(" is built for m <= 8 (m = 9, 10 take 32 lanes per problem)");
  if (desc->n > 64) return refuse(" is built for n <= 64");
  if (desc->trace != nullptr) return refuse(" records no per-iteration trace");
  if (desc->per_problem_data != nullptr)
    return refuse(" takes no per_problem_data: the caller's evaluation holds the problem's data");
  if (desc->hessian_from_functor) return refuse(": Lbfgsb has no preconditioned path (no hessian_from_functor)");
  if (desc->hessian_diagonal != nullptr) return refuse(": Lbfgsb has no preconditioned path (no hessian_diagonal)");
  if (desc->hessian_condition_stop > 0.0) return refuse(" computes no Hessian (no hessian_condition_stop)");
  if (desc->lanes_per_problem != 0 || desc->elems_per_lane != 0 || desc->history_placement != 0)
    return refuse(" chooses its own mapping: leave lanes_per_problem, elems_per_lane and history_placement 0");
  mi355_lbfgs_desc read = *desc;  // the objective is the caller's: its id and parameter fields are not looked at
  read.objective = MI355_OBJ_ROSENBROCK;
  read.objective_params = nullptr;
  read.n_params = 0;
  read.per_problem_stride = 0;
  return validate(ctx, &read, B);
}

ask_tell_box::Args step_args(const mi355_lbfgsb_ask_tell* h, const double* f, const double* g) {
  ask_tell_box::Args a;
  a.vectors = h->vectors;
  a.scalars = h->scalars;
  a.x_eval = h->x_eval;
  a.f = f;
  a.g = g;
  a.lower = h->lower;
  a.upper = h->upper;
  a.box_stride = h->box_stride;
  a.active = h->active;
  a.asks = h->asks;
  a.B = h->B;
  a.n = h->n;
  a.m = h->m;
  a.stop = h->stop;
  return a;
}

}  // namespace

extern "C" {

int mi355_lbfgsb_ask_tell_create(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, const double* lower,
                                 const double* upper, int64_t box_stride, int64_t B, const double* x0, void* stream_,
                                 mi355_lbfgsb_ask_tell** out) {
  if (!out) return fail(MI355_ERR_INVALID_ARGUMENT, "null handle pointer");
  *out = nullptr;
  const int rc = check(ctx, desc, B);
  if (rc != MI355_OK) return rc;
  if ((lower == nullptr) != (upper == nullptr))
    return fail(MI355_ERR_INVALID_ARGUMENT, "lower and upper must both be given or both be NULL");
  if (box_stride != 0 && !lower)
    return fail(MI355_ERR_INVALID_ARGUMENT, "per-problem bounds: lower and upper are required");
  if (box_stride != 0 && box_stride < desc->n)
    return fail(MI355_ERR_INVALID_ARGUMENT, "per-problem bounds: box_stride must be >= n (0: one shared box)");
  if (B > 0 && !x0) return fail(MI355_ERR_INVALID_ARGUMENT, "null x0");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(ctx);
  mi355_lbfgsb_ask_tell* h = new (std::nothrow) mi355_lbfgsb_ask_tell;
  if (!h) return fail(MI355_ERR_HIP, "ask/tell handle allocation failed");
  h->ctx = ctx;
  h->B = B;
  h->n = desc->n;
  h->m = desc->m;
  h->E = (desc->n <= 16) ? 1 : ((desc->n <= 32) ? 2 : 4);
  h->M = ask_tell_box_capacity(desc->m);
  h->stop = desc->stop;
  h->box_stride = (box_stride != 0) ? desc->n : 0;
  const size_t row = static_cast<size_t>(ask_tell_box::row_doubles(h->m, h->M, ask_tell_box::kLanes * h->E));
  const size_t eval_bytes = static_cast<size_t>(B) * h->n * sizeof(double);
  const size_t vector_bytes = static_cast<size_t>(B) * row * sizeof(double);
  const size_t scalar_bytes = static_cast<size_t>(B) * sizeof(ask_tell_box::Scalars);
  const size_t box_doubles = static_cast<size_t>(h->n) * ((box_stride != 0) ? static_cast<size_t>(B) : 1);
  const size_t counter_bytes = (1 + ask_tell_box::kAskKinds + 1) * sizeof(unsigned long long);
  h->bytes = eval_bytes + vector_bytes + scalar_bytes + 2 * box_doubles * sizeof(double) + counter_bytes;
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->block), h->bytes);
  if (e != hipSuccess) {
    const size_t asked = h->bytes;
    delete h;
    return fail(MI355_ERR_HIP, "hipMalloc of the ask/tell state (" + std::to_string(asked) + " bytes): " + hipGetErrorString(e));
  }
  char* p = h->block;
  h->x_eval = reinterpret_cast<double*>(p);
  p += eval_bytes;
  h->vectors = reinterpret_cast<double*>(p);
  p += vector_bytes;
  h->scalars = reinterpret_cast<ask_tell_box::Scalars*>(p);
  p += scalar_bytes;
  h->lower = reinterpret_cast<double*>(p);
  h->upper = h->lower + box_doubles;
  p += 2 * box_doubles * sizeof(double);
  h->active = reinterpret_cast<unsigned long long*>(p);
  h->asks = h->active + 1;
  h->nan_flag = reinterpret_cast<int*>(h->asks + ask_tell_box::kAskKinds);
  int status = MI355_OK;
  // padding, histories and scalars zero (phase: first evaluation pending), the counters too; every problem counts as
  // active
  hipError_t he = hipMemsetAsync(h->block + eval_bytes, 0, h->bytes - eval_bytes, stream);
  if (he == hipSuccess) {
    const unsigned long long all = static_cast<unsigned long long>(B);
    he = hipMemcpyAsync(h->active, &all, sizeof(all), hipMemcpyHostToDevice, stream);
  }
  if (he != hipSuccess) status = fail(MI355_ERR_HIP, std::string("ask/tell state initialisation: ") + hipGetErrorString(he));
  if (status == MI355_OK && B > 0) {
    ask_tell_box::InitArgs ia;
    ia.vectors = h->vectors;
    ia.scalars = h->scalars;
    ia.x_eval = h->x_eval;
    ia.x0 = x0;
    ia.lower = h->lower;
    ia.upper = h->upper;
    ia.lower_in = lower;
    ia.upper_in = upper;
    ia.box_stride_in = box_stride;
    ia.asks = h->asks;
    ia.nan_flag = h->nan_flag;
    ia.B = B;
    ia.row = static_cast<long long>(row);
    ia.n = h->n;
    status = dispatch_ask_tell_box_init(ia, stream);
    if (status == MI355_OK && lower != nullptr) {
      // a NaN bound makes the breakpoint order of the Cauchy search undefined in the reference as well (the check of
      // mi355_lbfgsb_minimize_batch_host, taken on the handle's copy: the caller's arrays are device memory here)
      int flag = 0;
      he = hipMemcpyAsync(&flag, h->nan_flag, sizeof(flag), hipMemcpyDeviceToHost, stream);
      if (he == hipSuccess) he = hipStreamSynchronize(stream);
      if (he != hipSuccess) status = fail(MI355_ERR_HIP, std::string("ask/tell box check: ") + hipGetErrorString(he));
      else if (flag != 0) status = fail(MI355_ERR_INVALID_ARGUMENT, "NaN bound");
    }
  }
  if (status != MI355_OK) {
    (void)hipFree(h->block);
    delete h;
    return status;
  }
  *out = h;
  return MI355_OK;
}

int mi355_lbfgsb_ask_tell_x(mi355_lbfgsb_ask_tell* handle, const double** x_eval) {
  if (!handle || !x_eval) return fail(MI355_ERR_INVALID_ARGUMENT, "null argument");
  *x_eval = handle->x_eval;
  return MI355_OK;
}

int mi355_lbfgsb_ask_tell_step(mi355_lbfgsb_ask_tell* handle, const double* f, const double* g, int64_t* active_host,
                               void* stream_) {
  if (!handle) return fail(MI355_ERR_INVALID_ARGUMENT, "null handle");
  if (handle->B > 0 && (!f || !g)) return fail(MI355_ERR_INVALID_ARGUMENT, "null f / g");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(handle->ctx);
  if (handle->B > 0) {
    const int rc = dispatch_ask_tell_box_step(handle->ctx, handle->E, step_args(handle, f, g), stream);
    if (rc != MI355_OK) return rc;
  }
  if (active_host) {
    unsigned long long count = 0;
    HIP_TRY(hipMemcpyAsync(&count, handle->active, sizeof(count), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *active_host = static_cast<int64_t>(count);
  }
  return MI355_OK;
}

int mi355_lbfgsb_ask_tell_active(mi355_lbfgsb_ask_tell* handle, const int64_t** active_dev) {
  if (!handle || !active_dev) return fail(MI355_ERR_INVALID_ARGUMENT, "null argument");
  *active_dev = reinterpret_cast<const int64_t*>(handle->active);
  return MI355_OK;
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
                                  mi355_lbfgs_progress* progress_out, void* stream_) {
  if (!handle) return fail(MI355_ERR_INVALID_ARGUMENT, "null handle");
  if (handle->B == 0) return MI355_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(handle->ctx);
  ask_tell_box::ResultArgs r;
  r.vectors = handle->vectors;
  r.scalars = handle->scalars;
  r.x_out = x_out;
  r.f_out = f_out;
  r.g_out = g_out;
  r.progress_out = progress_out;
  r.B = handle->B;
  r.row_p = static_cast<long long>(ask_tell_box::kLanes) * handle->E;
  r.row = ask_tell_box::row_doubles(handle->m, handle->M, ask_tell_box::kLanes * handle->E);
  r.n = handle->n;
  return dispatch_ask_tell_box_results(r, stream);
}

int mi355_lbfgsb_ask_tell_destroy(mi355_lbfgsb_ask_tell* handle) {
  if (!handle) return MI355_OK;
  MI355_ENTER_DEVICE(handle->ctx);
  const hipError_t e = hipFree(handle->block);  // (waits for the device: no kernel still reads the state)
  delete handle;
  if (e != hipSuccess) return fail(MI355_ERR_HIP, std::string("hipFree of the ask/tell state: ") + hipGetErrorString(e));
  return MI355_OK;
}

}  // extern "C"
