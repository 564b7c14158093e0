// ask_tell_host.hpp — the host code the four ask/tell (reverse communication) paths share: Lbfgs in double
// (mi355_lbfgs_ask_tell_*), Lbfgs in float (mi355_lbfgs_ask_tell_f32_*), Lbfgsb (mi355_lbfgsb_ask_tell_*) and Lbfgs in
// double above n = 256 (mi355_lbfgs_ask_tell_wide_*).  The
// handle base with its one device allocation, the refusals common to the three, the entry-point bodies
// (ask_tell_entry.hip turns them into the C functions), the two launches of the dispatch units and their choice among the
// built mappings.  No kernel lives here.
//
// A path is described by a traits struct T:
//   Scalar, Scalars, Args, ResultArgs   the types of its *_config.hpp
//   row(m, P)                           scalars of one problem's state row at padded width P
//   step(ctx, W, E, args, stream), results(result_args, stream)   the calls into its dispatch unit
//   listed_step(ctx, W, E, args, ids, listed, stream)             ... and into its unit of listed step kernels
//   kFinished                           the phase word of a finished problem (what a compaction drops)
//   kPrefix                             what its refusals start with ("Lbfgs ask/tell", ...)
//   kWhat                               how its HIP failures name the state ("ask/tell", "ask/tell f32")
// and by its public handle struct H, which derives from Handle<T> and, where the defaults of Handle do not do, adds the
// path's fields and its own kCounterWords, extra_bytes(), place_extras() and finish_args().
#pragma once
#include <memory>
#include <new>
#include <string>
#include <type_traits>

#include "engine_internal.hpp"

namespace mi355 {

// The compaction of a handle's list (ask_tell_compact_kernel.hpp, behind dispatch_ask_tell_compact.hip).
namespace ask_tell_compact {

constexpr int kGroup = 64;  // list entries per workgroup of the count and scatter kernels: one wavefront

template <class Scalar, class Scalars>
struct Args {
  const Scalars* scalars;  // [B], by problem: the phase words
  const long long* ids;    // [listed] the current list, ascending; nullptr: the identity (never compacted)
  long long* ids_next;     // [<= listed] the kept problems
  const Scalar* rows;      // [listed][n] the evaluation buffer, by slot
  Scalar* rows_next;       // [<= listed][n] the kept rows
  long long* counts;       // [groups + 1]: keep count per group, then their exclusive scan; [groups] = the total
  long long listed;
  int n;
};

}  // namespace ask_tell_compact

// the three launches; instantiated for the three wavefront paths in dispatch_ask_tell_compact.hip, specialised for the
// path above n = 256 in dispatch_lbfgs_ask_tell_wide_listed.hip
template <class Scalar, class Scalars, int kFinished>
int dispatch_ask_tell_compact(const ask_tell_compact::Args<Scalar, Scalars>& args, hipStream_t stream);

namespace ask_tell_host {

// One solve in flight: the state of all B problems in ONE device allocation,
//   [ vectors B row | x_eval B n | scalars B | the path's extras | counters: active, then the path's ]
// every part at a multiple of 16 bytes (carve()).  A handle that has been compacted (compact()) holds a second one,
//   [ ids B | ids B | rows B n | counts ceil(B / 64) + 1 ]
// the two id lists (the current one and the next), the packed rows of a compaction and its group counts.
template <class T>
struct Handle {
  using Traits = T;
  using Scalar = typename T::Scalar;
  mi355_lbfgs_ctx* ctx = nullptr;
  char* block = nullptr;
  size_t bytes = 0;
  Scalar* x_eval = nullptr;
  Scalar* vectors = nullptr;
  typename T::Scalars* scalars = nullptr;
  unsigned long long* active = nullptr;
  int64_t B = 0;
  int n = 0, m = 0, W = 0, E = 0;  // W lanes per problem at E coordinates per lane
  mi355_lbfgs_stop stop = {};
  // listed mode, from the first compact() on: slot s < listed of x_eval / f / g belongs to problem ids[s]
  bool listed_mode = false;
  int64_t listed = 0;
  char* list_block = nullptr;
  long long* ids = nullptr;  // the current list: one of ids_buffer; nullptr when B == 0
  long long* ids_buffer[2] = {nullptr, nullptr};
  Scalar* rows_next = nullptr;
  long long* counts = nullptr;

  // what a path without extras needs: the active counter alone, nothing between the scalars and the counters, and
  // step arguments that are the common ones
  static constexpr int kCounterWords = 1;
  size_t extra_bytes() const { return 0; }
  void place_extras(char*) {}
  void finish_args(typename T::Args&) const {}
};

template <class T>
int refuse(const char* text) {
  return fail(MI355_ERR_UNSUPPORTED, std::string(T::kPrefix) + text);
}

// Everything checked before the device is touched, in the order the paths have always reported it: the refusals
// (MI355_ERR_UNSUPPORTED, with the reason) — the shared ones here, the path's own in `before` and `after`, which stand
// where they stood in the path's sequence — then validate()'s argument checks on the fields the path reads (the
// objective and its parameters are not among them: the caller evaluates).
// allow_wide: validate()'s range of n ends at MI355_LBFGS_WIDE_MAX_N (the path above n = 256) instead of MI355_LBFGS_MAX_N.
template <class T, class Before, class After>
int check_common(const mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, Before before, After after,
                 bool allow_wide = false) {
  if (!ctx) return fail(MI355_ERR_INVALID_ARGUMENT, "null context");
  if (!desc) return fail(MI355_ERR_INVALID_ARGUMENT, "null desc");
  if (desc->linesearch == MI355_LS_HAGER_ZHANG)
    return refuse<T>(" is built with the More-Thuente line search only (no Hager-Zhang)");
  int rc = before();
  if (rc != MI355_OK) return rc;
  if (desc->trace != nullptr) return refuse<T>(" records no per-iteration trace");
  if (desc->per_problem_data != nullptr)
    return refuse<T>(" takes no per_problem_data: the caller's evaluation holds the problem's data");
  rc = after();
  if (rc != MI355_OK) return rc;
  mi355_lbfgs_desc read = *desc;  // the objective is the caller's: its id and parameter fields are not looked at
  read.objective = MI355_OBJ_ROSENBROCK;
  read.objective_params = nullptr;
  read.n_params = 0;
  read.per_problem_stride = 0;
  return validate(ctx, &read, B, allow_wide);
}

// The two Lbfgs paths: their refusals around the shared ones (T::kRefusesLargeM: the float path words the m limit
// itself, the double path leaves it to validate()), then the lane mapping — the caller's, or the narrowest built one
// that covers n.
template <class T>
int check_lbfgs(const mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, int& W, int& E) {
  const int rc = check_common<T>(
      ctx, desc, B,
      [&] {
        if (desc->arithmetic == MI355_ARITH_FMA)
          return refuse<T>(" is built for the exact arithmetic only (no MI355_ARITH_FMA)");
        if (desc->history_placement == MI355_HISTORY_Y_IN_REGISTERS)
          return refuse<T>(" keeps the history in device memory between calls (no MI355_HISTORY_Y_IN_REGISTERS)");
        if (desc->hessian_from_functor) return refuse<T>(" is built for First-mode functions (no hessian_from_functor)");
        if (desc->hessian_diagonal != nullptr) return refuse<T>(" is built for First-mode functions (no hessian_diagonal)");
        if (desc->hessian_condition_stop > 0.0)
          return refuse<T>(" is built for First-mode functions (no hessian_condition_stop)");
        return static_cast<int>(MI355_OK);
      },
      [&] {
        if (desc->n > MI355_LBFGS_MAX_N) return refuse<T>(" is built for n <= 256");
        if (T::kRefusesLargeM && desc->m > MI355_LBFGS_MAX_M) return refuse<T>(" is built for m <= 32 (MI355_LBFGS_MAX_M)");
        return static_cast<int>(MI355_OK);
      });
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
    return refuse<T>(": this mapping is not built; it must cover n with 8, 16, 32 or 64 lanes at one coordinate per lane, "
                     "or 64 lanes at two or four");
  return MI355_OK;
}

// The one layout of the three handles: byte offsets of the parts after the vectors (which start the block), each a
// multiple of 16, and the size of the whole.
struct Layout {
  size_t x_eval, scalars, extras, counters, bytes;
};

template <class H>
Layout carve(const H& h, size_t row) {
  using T = typename H::Traits;
  const auto round16 = [](size_t bytes) { return (bytes + 15) & ~static_cast<size_t>(15); };
  const size_t B = static_cast<size_t>(h.B);
  Layout l;
  l.x_eval = round16(B * row * sizeof(typename T::Scalar));
  l.scalars = l.x_eval + round16(B * h.n * sizeof(typename T::Scalar));
  l.extras = l.scalars + round16(B * sizeof(typename T::Scalars));
  l.counters = l.extras + round16(h.extra_bytes());
  l.bytes = l.counters + H::kCounterWords * sizeof(unsigned long long);
  return l;
}

template <class H>
typename H::Traits::Args step_args(const H* h, const typename H::Scalar* f, const typename H::Scalar* g) {
  typename H::Traits::Args a;
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
  h->finish_args(a);
  return a;
}

// check(H&): the path's checks; on MI355_OK it has set the path's mapping fields (and n-dependent extras) in the handle
// it was given.  init(H&, row, stream): the path's state initialisation launch, run when B > 0.
template <class H, class Check, class Init>
int create(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const typename H::Scalar* x0, void* stream_,
           H** out, Check check, Init init) {
  using T = typename H::Traits;
  if (!out) return fail(MI355_ERR_INVALID_ARGUMENT, "null handle pointer");
  *out = nullptr;
  H checked;
  const int rc = check(checked);
  if (rc != MI355_OK) return rc;
  if (B > 0 && !x0) return fail(MI355_ERR_INVALID_ARGUMENT, "null x0");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(ctx);
  const std::string what = T::kWhat;
  std::unique_ptr<H> h(new (std::nothrow) H(checked));
  if (!h) return fail(MI355_ERR_HIP, what + " handle allocation failed");
  h->ctx = ctx;
  h->B = B;
  h->n = desc->n;
  h->m = desc->m;
  h->stop = desc->stop;
  const size_t row = static_cast<size_t>(T::row(h->m, h->W * h->E));
  const Layout at = carve(*h, row);
  h->bytes = at.bytes;
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->block), h->bytes);
  if (e != hipSuccess)
    return fail(MI355_ERR_HIP, "hipMalloc of the " + what + " state (" + std::to_string(at.bytes) + " bytes): " + hipGetErrorString(e));
  h->vectors = reinterpret_cast<typename H::Scalar*>(h->block);
  h->x_eval = reinterpret_cast<typename H::Scalar*>(h->block + at.x_eval);
  h->scalars = reinterpret_cast<typename T::Scalars*>(h->block + at.scalars);
  h->active = reinterpret_cast<unsigned long long*>(h->block + at.counters);
  h->place_extras(h->block + at.extras);
  // everything zero: padding, histories and scalars (phase: first evaluation pending), the path's extras and counters;
  // then every problem counts as active
  hipError_t he = hipMemsetAsync(h->block, 0, h->bytes, stream);
  if (he == hipSuccess) {
    const unsigned long long all = static_cast<unsigned long long>(B);
    he = hipMemcpyAsync(h->active, &all, sizeof(all), hipMemcpyHostToDevice, stream);
  }
  int status = MI355_OK;
  if (he != hipSuccess) status = fail(MI355_ERR_HIP, what + " state initialisation: " + hipGetErrorString(he));
  if (status == MI355_OK && B > 0) status = init(*h, static_cast<long long>(row), stream);
  if (status != MI355_OK) {
    (void)hipFree(h->block);
    return status;
  }
  *out = h.release();
  return MI355_OK;
}

template <class H>
int x(H* handle, const typename H::Scalar** x_eval) {
  if (!handle || !x_eval) return fail(MI355_ERR_INVALID_ARGUMENT, "null argument");
  *x_eval = handle->x_eval;
  return MI355_OK;
}

template <class H>
int step(H* handle, const typename H::Scalar* f, const typename H::Scalar* g, int64_t* active_host, void* stream_) {
  if (!handle) return fail(MI355_ERR_INVALID_ARGUMENT, "null handle");
  // the rows the caller evaluated: all B, or the list of a compacted handle (f [listed], g [listed][n])
  const int64_t rows = handle->listed_mode ? handle->listed : handle->B;
  if (rows > 0 && (!f || !g)) return fail(MI355_ERR_INVALID_ARGUMENT, "null f / g");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(handle->ctx);
  if (rows > 0) {
    const int rc = handle->listed_mode
                       ? H::Traits::listed_step(handle->ctx, handle->W, handle->E, step_args(handle, f, g), handle->ids,
                                                handle->listed, stream)
                       : H::Traits::step(handle->ctx, handle->W, handle->E, step_args(handle, f, g), stream);
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

// The second allocation of a handle, made at its first compaction.  On failure the handle is as it was.
template <class H>
int allocate_list(H* h) {
  const auto round16 = [](size_t bytes) { return (bytes + 15) & ~static_cast<size_t>(15); };
  const size_t B = static_cast<size_t>(h->B);
  const size_t id_bytes = round16(B * sizeof(long long));
  const size_t row_bytes = round16(B * h->n * sizeof(typename H::Scalar));
  const size_t groups = (B + ask_tell_compact::kGroup - 1) / ask_tell_compact::kGroup;
  const size_t bytes = 2 * id_bytes + row_bytes + (groups + 1) * sizeof(long long);
  char* block = nullptr;
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&block), bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(MI355_ERR_HIP, std::string("hipMalloc of the ") + H::Traits::kWhat + " list (" + std::to_string(bytes) +
                                   " bytes): " + hipGetErrorString(e));
  }
  h->list_block = block;
  h->ids_buffer[0] = reinterpret_cast<long long*>(block);
  h->ids_buffer[1] = reinterpret_cast<long long*>(block + id_bytes);
  h->rows_next = reinterpret_cast<typename H::Scalar*>(block + 2 * id_bytes);
  h->counts = reinterpret_cast<long long*>(block + 2 * id_bytes + row_bytes);
  return MI355_OK;
}

// Rebuilds the list: of the problems listed now (all B before the first call), those that have not finished, in
// ascending order, with their rows of x_eval packed to the front.  Waits for the stream; from here on the handle is in
// listed mode.
template <class H>
int compact(H* handle, int64_t* listed_host, void* stream_) {
  using T = typename H::Traits;
  if (!handle || !listed_host) return fail(MI355_ERR_INVALID_ARGUMENT, "null argument");
  const int64_t current = handle->listed_mode ? handle->listed : handle->B;
  if (current == 0) {  // an empty batch, or everything has finished: nothing to launch
    handle->listed_mode = true;
    handle->listed = 0;
    *listed_host = 0;
    return MI355_OK;
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(handle->ctx);
  if (!handle->list_block) {
    const int rc = allocate_list(handle);
    if (rc != MI355_OK) return rc;
  }
  long long* const next = (handle->ids == handle->ids_buffer[0]) ? handle->ids_buffer[1] : handle->ids_buffer[0];
  ask_tell_compact::Args<typename H::Scalar, typename T::Scalars> a;
  a.scalars = handle->scalars;
  a.ids = handle->listed_mode ? handle->ids : nullptr;
  a.ids_next = next;
  a.rows = handle->x_eval;
  a.rows_next = handle->rows_next;
  a.counts = handle->counts;
  a.listed = current;
  a.n = handle->n;
  const int rc = dispatch_ask_tell_compact<typename H::Scalar, typename T::Scalars, T::kFinished>(a, stream);
  if (rc != MI355_OK) return rc;
  const long long groups = (current + ask_tell_compact::kGroup - 1) / ask_tell_compact::kGroup;
  long long total = 0;
  HIP_TRY(hipMemcpyAsync(&total, handle->counts + groups, sizeof(total), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (total < 0 || total > current) return fail(MI355_ERR_HIP, "internal: the compaction kept more than was listed");
  if (total > 0)  // the packed rows back into the evaluation buffer, whose pointer the caller holds
    HIP_TRY(hipMemcpyAsync(handle->x_eval, handle->rows_next,
                           static_cast<size_t>(total) * handle->n * sizeof(typename H::Scalar), hipMemcpyDeviceToDevice,
                           stream));
  handle->ids = next;
  handle->listed = total;
  handle->listed_mode = true;
  *listed_host = total;
  return MI355_OK;
}

// The list of a compacted handle: DEVICE [listed], ascending.  Before the first compaction: nullptr and B.
template <class H>
int ids(H* handle, const int64_t** ids_dev, int64_t* listed) {
  if (!handle || !ids_dev || !listed) return fail(MI355_ERR_INVALID_ARGUMENT, "null argument");
  static_assert(sizeof(long long) == sizeof(int64_t), "the list is handed out as int64_t");
  *ids_dev = handle->listed_mode ? reinterpret_cast<const int64_t*>(handle->ids) : nullptr;
  *listed = handle->listed_mode ? handle->listed : handle->B;
  return MI355_OK;
}

template <class H>
int active(H* handle, const int64_t** active_dev) {
  if (!handle || !active_dev) return fail(MI355_ERR_INVALID_ARGUMENT, "null argument");
  *active_dev = reinterpret_cast<const int64_t*>(handle->active);
  return MI355_OK;
}

template <class H>
int results(H* handle, typename H::Scalar* x_out, typename H::Scalar* f_out, typename H::Scalar* g_out,
            mi355_lbfgs_progress* progress_out, void* stream_) {
  using T = typename H::Traits;
  if (!handle) return fail(MI355_ERR_INVALID_ARGUMENT, "null handle");
  if (handle->B == 0) return MI355_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MI355_ENTER_DEVICE(handle->ctx);
  typename T::ResultArgs r;
  r.vectors = handle->vectors;
  r.scalars = handle->scalars;
  r.x_out = x_out;
  r.f_out = f_out;
  r.g_out = g_out;
  r.progress_out = progress_out;
  r.B = handle->B;
  r.row_p = static_cast<long long>(handle->W) * handle->E;
  r.row = T::row(handle->m, handle->W * handle->E);
  r.n = handle->n;
  return T::results(r, stream);
}

template <class H>
int destroy(H* handle) {
  if (!handle) return MI355_OK;
  MI355_ENTER_DEVICE(handle->ctx);
  hipError_t e = hipFree(handle->block);  // (waits for the device: no kernel still reads the state)
  const hipError_t e_list = hipFree(handle->list_block);  // (nullptr: a handle that was never compacted)
  if (e == hipSuccess) e = e_list;
  delete handle;
  if (e != hipSuccess)
    return fail(MI355_ERR_HIP, std::string("hipFree of the ") + H::Traits::kWhat + " state: " + hipGetErrorString(e));
  return MI355_OK;
}

}  // namespace ask_tell_host

// The step launch of the three dispatch units.  kern: a __global__ function taking the path's Args, one wavefront per
// workgroup, W lanes per problem at E coordinates per lane; dynamic_lds: its dynamic LDS bytes (0: none, and the
// kernel's limit is left alone); reported_lds: what last_launch() says (the static LDS of a kernel without dynamic).
// A grid-stride loop over `rows` rows of the caller's arrays — the batch, or the list of a compacted handle, whose
// kernel takes the list after the path's Args (`more`) —: as many workgroups as the chip holds (or the rows need).
template <int W, int E, class Kernel, class Args, class... More>
int launch_ask_tell_rows(mi355_lbfgs_ctx* ctx, Kernel kern, int dynamic_lds, int reported_lds, long long rows,
                         const Args& args, hipStream_t stream, const More&... more) {
  constexpr int kSegs = kWave / W;
  if (args.n > W * E) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the lane mapping does not cover n");
  if (rows < 1 || rows > args.B) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: the rows of a step do not fit the batch");
  if (dynamic_lds > 0)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, dynamic_lds));
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWave, dynamic_lds));
  if (per_cu < 1) per_cu = 1;
  const long long blocks_needed = (rows + kSegs - 1) / kSegs;
  long long blocks_ll = static_cast<long long>(per_cu) * ctx->num_cus;
  if (ctx->debug_blocks >= 1 && ctx->debug_blocks < blocks_ll) blocks_ll = ctx->debug_blocks;
  if (blocks_ll > blocks_needed) blocks_ll = blocks_needed;
  HIP_TRY(hipMemsetAsync(args.active, 0, sizeof(unsigned long long), stream));
  HIP_TRY(hipEventRecord(ctx->ev_start, stream));
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks_ll)), dim3(kWave), dynamic_lds, stream, args, more...);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ev_stop, stream));
  ctx->timed = true;
  ctx->last_W = W;
  ctx->last_E = E;
  ctx->last_blocks = static_cast<int>(blocks_ll);
  ctx->last_threads = kWave;
  ctx->last_lds = reported_lds;
  ctx->last_mr = 0;
  ctx->last_variant = MI355_KERNEL_GENERAL;
  ctx->last_arith = MI355_ARITH_EXACT;
  return MI355_OK;
}

// ... over the whole batch: the step of a handle that has not been compacted
template <int W, int E, class Kernel, class Args>
int launch_ask_tell_step(mi355_lbfgs_ctx* ctx, Kernel kern, int dynamic_lds, int reported_lds, const Args& args,
                         hipStream_t stream) {
  return launch_ask_tell_rows<W, E>(ctx, kern, dynamic_lds, reported_lds, args.B, args, stream);
}

// ... over the list of a compacted handle: kern takes the list after the path's Args and reads its length from Args::B
template <int W, int E, class Kernel, class Args>
int launch_ask_tell_listed(mi355_lbfgs_ctx* ctx, Kernel kern, int dynamic_lds, int reported_lds, const Args& args,
                           const long long* ids, long long listed, hipStream_t stream) {
  if (!ids || listed > args.B) return fail(MI355_ERR_INVALID_ARGUMENT, "internal: a listed step without a list");
  Args rows = args;
  rows.B = listed;
  return launch_ask_tell_rows<W, E>(ctx, kern, dynamic_lds, reported_lds, listed, rows, stream, ids);
}

// launch(std::integral_constant<int, W>(), std::integral_constant<int, E>()) for the mapping of the call, one of the six
// the two Lbfgs paths build: 8, 16, 32 or 64 lanes per problem at one coordinate per lane, 64 lanes at two or four.
// none: the "internal:" line for any other.
template <class Launch>
int launch_for_lbfgs_mapping(int W, int E, const char* none, Launch launch) {
  using One = std::integral_constant<int, 1>;
  using Wave = std::integral_constant<int, 64>;
  if (E == 1) {
    switch (W) {
      case 8: return launch(std::integral_constant<int, 8>(), One());
      case 16: return launch(std::integral_constant<int, 16>(), One());
      case 32: return launch(std::integral_constant<int, 32>(), One());
      case 64: return launch(Wave(), One());
    }
  }
  if (W == 64 && E == 2) return launch(Wave(), std::integral_constant<int, 2>());
  if (W == 64 && E == 4) return launch(Wave(), std::integral_constant<int, 4>());
  return fail(MI355_ERR_UNSUPPORTED, none);
}

// launch(std::integral_constant<int, E>(), std::integral_constant<int, M>()) for the Lbfgsb path: one, two or four
// coordinates per lane of its sixteen-lane segment at history capacity M = 5 or 8 (`capacity`: ask_tell_box_capacity(m))
template <class Launch>
int launch_for_box_mapping(int E, int capacity, Launch launch) {
  const auto at = [&](auto e) {
    if (capacity == 5) return launch(e, std::integral_constant<int, 5>());
    return launch(e, std::integral_constant<int, 8>());
  };
  switch (E) {
    case 1: return at(std::integral_constant<int, 1>());
    case 2: return at(std::integral_constant<int, 2>());
    case 4: return at(std::integral_constant<int, 4>());
  }
  return fail(MI355_ERR_UNSUPPORTED, "internal: no Lbfgsb ask/tell kernel for this number of coordinates per lane");
}

// kern(args...) with one thread per element, `total` = B n of them: the state initialisations and the result gathers
template <class Kernel, class... A>
int launch_elementwise(Kernel kern, long long total, hipStream_t stream, const A&... args) {
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, args...);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}

}  // namespace mi355
