// ask_tell_f32_entry.hip — the C entry points of the float ask/tell (reverse communication) L-BFGS
// (include/mi355_lbfgs.h, mi355_lbfgs_ask_tell_f32_*): the refusals, the solve handle with its one device allocation, and
// the calls into dispatch_lbfgs_ask_tell_f32.hip.  No kernel lives here.
#include <new>

#include "engine_internal.hpp"
#include "lbfgs_ask_tell_f32_config.hpp"

using namespace mi355;

// One solve in flight: the state of all B problems in ONE device allocation, every part at a multiple of 16 bytes
//   [ vectors B (3 + 2m) P | x_eval B n | scalars B | active counter ]
struct mi355_lbfgs_ask_tell_f32 {
  mi355_lbfgs_ctx* ctx = nullptr;
  char* block = nullptr;
  size_t bytes = 0;
  float* x_eval = nullptr;
  float* vectors = nullptr;
  ask_tell_f32::Scalars* scalars = nullptr;
  unsigned long long* active = nullptr;
  int64_t B = 0;
  int n = 0, m = 0, W = 0, E = 0;
  mi355_lbfgs_stop stop;
};

namespace {

int refuse(const char* text) { return fail(MI355_ERR_UNSUPPORTED, std::string("Lbfgs ask/tell f32") + text); }

size_t round16(size_t bytes) { return (bytes + 15) & ~static_cast<size_t>(15); }

// Everything checked before the device is touched: the refusals (MI355_ERR_UNSUPPORTED, with the reason), then
// validate()'s argument checks on the fields this path reads (the objective and its parameters are not among them: the
// caller evaluates), then the lane mapping.
int check(const mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, int& W, int& E) {
  if (!ctx) return fail(MI355_ERR_INVALID_ARGUMENT, "null context");
  if (!desc) return fail(MI355_ERR_INVALID_ARGUMENT, "null desc");
  if (desc->linesearch == MI355_LS_HAGER_ZHANG)
    return refuse(" is built with the More-Thuente line search only (no Hager-Zhang)");
  if (desc->arithmetic == MI355_ARITH_FMA) return refuse(" is built for the exact arithmetic only (no MI355_ARITH_FMA)");
  if (desc->history_placement == MI355_HISTORY_Y_IN_REGISTERS)
    return refuse(" keeps the history in device memory between calls (no MI355_HISTORY_Y_IN_REGISTERS)");
  if (desc->hessian_from_functor) return refuse(" is built for First-mode functions (no hessian_from_functor)");
  if (desc->hessian_diagonal != nullptr) return refuse(" is built for First-mode functions (no hessian_diagonal)");
  if (desc->hessian_condition_stop > 0.0)
    return refuse(" is built for First-mode functions (no hessian_condition_stop)");
  if (desc->trace != nullptr) return refuse(" records no per-iteration trace");
  if (desc->per_problem_data != nullptr)
    return refuse(" takes no per_problem_data: the caller's evaluation holds the problem's data");
  if (desc->n > MI355_LBFGS_MAX_N) return refuse(" is built for n <= 256");
  if (desc->m > MI355_LBFGS_MAX_M) return refuse(" is built for m <= 32 (MI355_LBFGS_MAX_M)");
  mi355_lbfgs_desc read = *desc;  // the objective is the caller's: its id and parameter fields are not looked at
  read.objective = MI355_OBJ_ROSENBROCK;
  read.objective_params = nullptr;
  read.n_params = 0;
  read.per_problem_stride = 0;
  const int rc = validate(ctx, &read, B);
  if (rc != MI355_OK) return rc;
  W = desc->lanes_per_problem;
  E = desc->elems_per_lane;
  if (W == 0 && E == 0) {
    W = 8;
    while (W < desc->n && W < 64) W <<= 1;
  }
  if (E == 0 && (W == 8 || W == 16 || W == 32 || W == 64)) E = (desc->n <= W) ? 1 : ((desc->n <= 2 * W) ? 2 : 4);
  const bool built = ((W == 8 || W == 16 || W == 32 || W == 64) && E == 1) || (W == 64 && (E == 2 || E == 4));
  if (!built || W * E < desc->n)
    return refuse(": this mapping is not built; it must cover n with 8, 16, 32 or 64 lanes at one coordinate per lane, "
                  "or 64 lanes at two or four");
  return MI355_OK;
}

ask_tell_f32::Args step_args(const mi355_lbfgs_ask_tell_f32* h, const float* f, const float* g) {
  ask_tell_f32::Args a;
  a.vectors = h->vectors;
  a.scalars = h->scalars;
  a.x_eval = h->x_eval;
  a.f = f;
  a.g = g;
  a.active = h->active;
  a.B = h->B;
  a.n = h->n;
  a.m = h->m;
  a.stop = h->stop;
  a.stop_x_delta = static_cast<float>(h->stop.x_delta);
  a.stop_f_delta = static_cast<float>(h->stop.f_delta);
  a.stop_gradient_norm = static_cast<float>(h->stop.gradient_norm);
  a.stop_past_delta = static_cast<float>(h->stop.past_delta);
  return a;
}

}  // namespace

extern "C" {

int mi355_lbfgs_ask_tell_f32_create(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const float* x0,
                                    void* stream_, mi355_lbfgs_ask_tell_f32** out) {
  if (!out) return fail(MI355_ERR_INVALID_ARGUMENT, "null handle pointer");
  *out = nullptr;
  int W = 0, E = 0;
  const int rc = check(ctx, desc, B, W, E);
  if (rc != MI355_OK) return rc;
  if (B > 0 && !x0) return fail(MI355_ERR_INVALID_ARGUMENT, "null x0");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(ctx);
  mi355_lbfgs_ask_tell_f32* h = new (std::nothrow) mi355_lbfgs_ask_tell_f32;
  if (!h) return fail(MI355_ERR_HIP, "ask/tell f32 handle allocation failed");
  h->ctx = ctx;
  h->B = B;
  h->n = desc->n;
  h->m = desc->m;
  h->W = W;
  h->E = E;
  h->stop = desc->stop;
  const size_t row = static_cast<size_t>(ask_tell_f32::row_floats(h->m, W * E));
  const size_t vector_bytes = round16(static_cast<size_t>(B) * row * sizeof(float));
  const size_t eval_bytes = round16(static_cast<size_t>(B) * h->n * sizeof(float));
  const size_t scalar_bytes = round16(static_cast<size_t>(B) * sizeof(ask_tell_f32::Scalars));
  h->bytes = vector_bytes + eval_bytes + scalar_bytes + sizeof(unsigned long long);
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->block), h->bytes);
  if (e != hipSuccess) {
    const size_t asked = h->bytes;
    delete h;
    return fail(MI355_ERR_HIP, "hipMalloc of the ask/tell f32 state (" + std::to_string(asked) + " bytes): " + hipGetErrorString(e));
  }
  h->vectors = reinterpret_cast<float*>(h->block);
  h->x_eval = reinterpret_cast<float*>(h->block + vector_bytes);
  h->scalars = reinterpret_cast<ask_tell_f32::Scalars*>(h->block + vector_bytes + eval_bytes);
  h->active = reinterpret_cast<unsigned long long*>(h->block + vector_bytes + eval_bytes + scalar_bytes);
  int status = MI355_OK;
  // everything zero: padding, rings and scalars (phase: first evaluation pending); every problem counts as active
  hipError_t he = hipMemsetAsync(h->block, 0, vector_bytes + eval_bytes + scalar_bytes, stream);
  if (he == hipSuccess) {
    const unsigned long long all = static_cast<unsigned long long>(B);
    he = hipMemcpyAsync(h->active, &all, sizeof(all), hipMemcpyHostToDevice, stream);
  }
  if (he != hipSuccess) status = fail(MI355_ERR_HIP, std::string("ask/tell f32 state initialisation: ") + hipGetErrorString(he));
  if (status == MI355_OK && B > 0)
    status = dispatch_ask_tell_f32_init(step_args(h, nullptr, nullptr), x0, static_cast<long long>(row), stream);
  if (status != MI355_OK) {
    (void)hipFree(h->block);
    delete h;
    return status;
  }
  *out = h;
  return MI355_OK;
}

int mi355_lbfgs_ask_tell_f32_x(mi355_lbfgs_ask_tell_f32* handle, const float** x_eval) {
  if (!handle || !x_eval) return fail(MI355_ERR_INVALID_ARGUMENT, "null argument");
  *x_eval = handle->x_eval;
  return MI355_OK;
}

int mi355_lbfgs_ask_tell_f32_step(mi355_lbfgs_ask_tell_f32* handle, const float* f, const float* g,
                                  int64_t* active_host, void* stream_) {
  if (!handle) return fail(MI355_ERR_INVALID_ARGUMENT, "null handle");
  if (handle->B > 0 && (!f || !g)) return fail(MI355_ERR_INVALID_ARGUMENT, "null f / g");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(handle->ctx);
  if (handle->B > 0) {
    const int rc = dispatch_ask_tell_f32_step(handle->ctx, handle->W, handle->E, step_args(handle, f, g), stream);
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

int mi355_lbfgs_ask_tell_f32_active(mi355_lbfgs_ask_tell_f32* handle, const int64_t** active_dev) {
  if (!handle || !active_dev) return fail(MI355_ERR_INVALID_ARGUMENT, "null argument");
  *active_dev = reinterpret_cast<const int64_t*>(handle->active);
  return MI355_OK;
}

int mi355_lbfgs_ask_tell_f32_results(mi355_lbfgs_ask_tell_f32* handle, float* x_out, float* f_out, float* g_out,
                                     mi355_lbfgs_progress* progress_out, void* stream_) {
  if (!handle) return fail(MI355_ERR_INVALID_ARGUMENT, "null handle");
  if (handle->B == 0) return MI355_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(handle->ctx);
  ask_tell_f32::ResultArgs r;
  r.vectors = handle->vectors;
  r.scalars = handle->scalars;
  r.x_out = x_out;
  r.f_out = f_out;
  r.g_out = g_out;
  r.progress_out = progress_out;
  r.B = handle->B;
  r.row_p = static_cast<long long>(handle->W) * handle->E;
  r.row = ask_tell_f32::row_floats(handle->m, handle->W * handle->E);
  r.n = handle->n;
  return dispatch_ask_tell_f32_results(r, stream);
}

int mi355_lbfgs_ask_tell_f32_destroy(mi355_lbfgs_ask_tell_f32* handle) {
  if (!handle) return MI355_OK;
  MI355_ENTER_DEVICE(handle->ctx);
  const hipError_t e = hipFree(handle->block);  // (waits for the device: no kernel still reads the state)
  delete handle;
  if (e != hipSuccess) return fail(MI355_ERR_HIP, std::string("hipFree of the ask/tell f32 state: ") + hipGetErrorString(e));
  return MI355_OK;
}

}  // extern "C"
