// cppoptlib/mi355/ask_tell.h — Lbfgs<F, m, MoreThuente> for an objective the CALLER evaluates on the device, without a
// device functor and without a second build of the library: reverse communication (ask / tell) over the C entry points
// mi355_lbfgs_ask_tell_* (include/mi355_lbfgs.h has the protocol).
//
//   LbfgsAskTell        RAII handle of one batched solve: Ask() is the device pointer of the points to evaluate
//                       ([B][n], the same pointer for the handle's lifetime), Tell(f_dev, g_dev) hands the values and
//                       gradients back and returns the number of problems still active, Results(...) copies the states.
//                       The dimension picks the C handle: mi355_lbfgs_ask_tell_* up to n = 256, above it
//                       mi355_lbfgs_ask_tell_wide_* (a workgroup per problem; the library's mapping only;
//                       B ((3 + 2 m) n + n) 8 bytes of device memory).  MinimizeBatchWith and
//                       MinimizeBatchWithCompaction follow, being loops over the handle.
//   LbfgsAskTellF32     the same in native float (mi355_lbfgs_ask_tell_f32_*): float x0, points, values, gradients and
//                       results — a float objective is evaluated in its own precision, never widened
//   LbfgsbAskTell       the same for Lbfgsb<F, m, MoreThuente>: no box, one shared box, or one box per problem
//                       (mi355_lbfgsb_ask_tell_*), plus Asks(), the count of every kind of evaluation asked for
//   MinimizeBatchWith   the loop around either: evaluator(x_dev, f_dev, g_dev, B, n) is the user's — its own kernels,
//                       hipBLAS, anything that leaves f [B] and g [B][n] in device memory, ordered on `stream`.
//   Compact(), Ids()    on the three handles: the listed mode (mi355_ask_tell_compact_*), in which the caller evaluates
//                       only the problems that have not finished; MinimizeBatchWithCompaction is the loop around it.
//
// Plain C++17: no HIP header is needed here; the device arrays are the caller's.  Failures surface through Fail()
// (context.h): an exception, or abort() when built with -fno-exceptions.
#ifndef CPPOPTLIB_MI355_ASK_TELL_H_
#define CPPOPTLIB_MI355_ASK_TELL_H_

#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <utility>

#include "context.h"

namespace cppoptlib::mi355 {

// The fields of mi355_lbfgs_desc the ask/tell path reads, with the reference's defaults (Lbfgs's m = 10,
// DefaultStoppingSolverProgress); everything else of the desc stays zero.
inline mi355_lbfgs_desc AskTellDesc(int n, int m = 10, const mi355_lbfgs_stop* stop = nullptr, int lanes_per_problem = 0,
                                    int elems_per_lane = 0) {
  mi355_lbfgs_desc d = {};
  d.objective = MI355_OBJ_ROSENBROCK;  // not read: the caller evaluates
  d.linesearch = MI355_LS_MORE_THUENTE;
  d.n = n;
  d.m = m;
  d.lanes_per_problem = lanes_per_problem;
  d.elems_per_lane = elems_per_lane;
  d.arithmetic = MI355_ARITH_EXACT;
  if (stop != nullptr) {
    d.stop = *stop;
  } else {
    Check(mi355_lbfgs_default_stop(0, &d.stop), "mi355_lbfgs_default_stop");
  }
  return d;
}

namespace detail {

// What tells the three C handle types apart: the scalar, the handle, its C functions, and the names a failure reports
// (the class for a null context, "<kPrefix><function>" for a C call).
// What LbfgsAskTell holds: the C handle its dimension selects — mi355_lbfgs_ask_tell up to n = MI355_LBFGS_MAX_N (a
// wavefront segment per problem), mi355_lbfgs_ask_tell_wide above (a workgroup per problem).  Exactly one is set.
struct LbfgsAskTellByDimension {
  mi355_lbfgs_ask_tell* narrow = nullptr;
  mi355_lbfgs_ask_tell_wide* wide = nullptr;
};
struct LbfgsAskTellApi {
  using Scalar = double;
  using Handle = LbfgsAskTellByDimension;
  static int create(mi355_lbfgs_ctx* ctx, const mi355_lbfgs_desc* desc, int64_t B, const double* x0, void* stream,
                    Handle** out) {
    *out = nullptr;
    Handle* h = new (std::nothrow) Handle;
    if (h == nullptr) Fail("LbfgsAskTell: out of memory");
    const int rc = (desc != nullptr && desc->n > MI355_LBFGS_MAX_N)
                       ? mi355_lbfgs_ask_tell_wide_create(ctx, desc, B, x0, stream, &h->wide)
                       : mi355_lbfgs_ask_tell_create(ctx, desc, B, x0, stream, &h->narrow);
    if (rc != MI355_OK) {
      delete h;
      return rc;
    }
    *out = h;
    return rc;
  }
  static int x(Handle* h, const double** x_eval) {
    return h->wide ? mi355_lbfgs_ask_tell_wide_x(h->wide, x_eval) : mi355_lbfgs_ask_tell_x(h->narrow, x_eval);
  }
  static int step(Handle* h, const double* f, const double* g, int64_t* active_host, void* stream) {
    return h->wide ? mi355_lbfgs_ask_tell_wide_step(h->wide, f, g, active_host, stream)
                   : mi355_lbfgs_ask_tell_step(h->narrow, f, g, active_host, stream);
  }
  static int active(Handle* h, const int64_t** active_dev) {
    return h->wide ? mi355_lbfgs_ask_tell_wide_active(h->wide, active_dev) : mi355_lbfgs_ask_tell_active(h->narrow, active_dev);
  }
  static int results(Handle* h, double* x_out, double* f_out, double* g_out, mi355_lbfgs_progress* progress_out,
                     void* stream) {
    return h->wide ? mi355_lbfgs_ask_tell_wide_results(h->wide, x_out, f_out, g_out, progress_out, stream)
                   : mi355_lbfgs_ask_tell_results(h->narrow, x_out, f_out, g_out, progress_out, stream);
  }
  static int destroy(Handle* h) {
    if (h == nullptr) return MI355_OK;
    const int rc = h->wide ? mi355_lbfgs_ask_tell_wide_destroy(h->wide) : mi355_lbfgs_ask_tell_destroy(h->narrow);
    delete h;
    return rc;
  }
  static int compact(Handle* h, int64_t* listed_host, void* stream) {
    return h->wide ? mi355_lbfgs_ask_tell_wide_compact(h->wide, listed_host, stream)
                   : mi355_ask_tell_compact_lbfgs(h->narrow, listed_host, stream);
  }
  static int ids(Handle* h, const int64_t** ids_dev, int64_t* listed) {
    return h->wide ? mi355_lbfgs_ask_tell_wide_ids(h->wide, ids_dev, listed) : mi355_ask_tell_ids_lbfgs(h->narrow, ids_dev, listed);
  }
  static constexpr const char* kClass = "LbfgsAskTell";
  static constexpr const char* kPrefix = "mi355_lbfgs_ask_tell_";
};
struct LbfgsAskTellF32Api {
  using Scalar = float;
  using Handle = mi355_lbfgs_ask_tell_f32;
  static constexpr auto create = &mi355_lbfgs_ask_tell_f32_create;
  static constexpr auto x = &mi355_lbfgs_ask_tell_f32_x;
  static constexpr auto step = &mi355_lbfgs_ask_tell_f32_step;
  static constexpr auto active = &mi355_lbfgs_ask_tell_f32_active;
  static constexpr auto results = &mi355_lbfgs_ask_tell_f32_results;
  static constexpr auto destroy = &mi355_lbfgs_ask_tell_f32_destroy;
  static constexpr auto compact = &mi355_ask_tell_compact_lbfgs_f32;
  static constexpr auto ids = &mi355_ask_tell_ids_lbfgs_f32;
  static constexpr const char* kClass = "LbfgsAskTellF32";
  static constexpr const char* kPrefix = "mi355_lbfgs_ask_tell_f32_";
};
struct LbfgsbAskTellApi {
  using Scalar = double;
  using Handle = mi355_lbfgsb_ask_tell;
  static constexpr auto create = &mi355_lbfgsb_ask_tell_create;
  static constexpr auto x = &mi355_lbfgsb_ask_tell_x;
  static constexpr auto step = &mi355_lbfgsb_ask_tell_step;
  static constexpr auto active = &mi355_lbfgsb_ask_tell_active;
  static constexpr auto results = &mi355_lbfgsb_ask_tell_results;
  static constexpr auto destroy = &mi355_lbfgsb_ask_tell_destroy;
  static constexpr auto compact = &mi355_ask_tell_compact_lbfgsb;
  static constexpr auto ids = &mi355_ask_tell_ids_lbfgsb;
  static constexpr const char* kClass = "LbfgsbAskTell";
  static constexpr const char* kPrefix = "mi355_lbfgsb_ask_tell_";
};

// The RAII handle of one batched solve over the C handle of `Api`: what LbfgsAskTell, LbfgsAskTellF32 and LbfgsbAskTell are.
template <class Api>
class AskTellHandle {
 public:
  using Scalar = typename Api::Scalar;
  // x0_dev: DEVICE [B][n] of Scalar.  stream: a hipStream_t (nullptr: the default stream) for this and every later call.
  AskTellHandle(std::shared_ptr<Context> context, const mi355_lbfgs_desc& desc, int64_t B, const Scalar* x0_dev,
                void* stream = nullptr)
      : AskTellHandle(std::move(context), desc.n, B, stream, [&](mi355_lbfgs_ctx* ctx, typename Api::Handle** out) {
          return Api::create(ctx, &desc, B, x0_dev, stream, out);
        }) {}
  ~AskTellHandle() { (void)Api::destroy(handle_); }
  AskTellHandle(const AskTellHandle&) = delete;
  AskTellHandle& operator=(const AskTellHandle&) = delete;
  AskTellHandle(AskTellHandle&& other) noexcept
      : context_(std::move(other.context_)), handle_(other.handle_), x_(other.x_), stream_(other.stream_), B_(other.B_),
        n_(other.n_) {
    other.handle_ = nullptr;
  }
  AskTellHandle& operator=(AskTellHandle&&) = delete;

  // DEVICE [B][n]: the points to evaluate (rows of finished problems hold their returned x)
  const Scalar* Ask() const { return x_; }
  // f_dev [B], g_dev [B][n]: the evaluation of Ask()'s rows.  Waits for the stream; returns the problems still active.
  int64_t Tell(const Scalar* f_dev, const Scalar* g_dev) {
    int64_t active = 0;
    Checked(Api::step(handle_, f_dev, g_dev, &active, stream_), "step");
    return active;
  }
  // ... without waiting: the count is behind ActiveDevice() once the stream has run the call
  void TellAsync(const Scalar* f_dev, const Scalar* g_dev) {
    Checked(Api::step(handle_, f_dev, g_dev, nullptr, stream_), "step");
  }
  const int64_t* ActiveDevice() const {
    const int64_t* p = nullptr;
    Checked(Api::active(handle_, &p), "active");
    return p;
  }
  // The current iterate of every problem, its value, gradient and progress record into DEVICE arrays (any may be null);
  // asynchronous on the stream.
  void Results(Scalar* x_dev, Scalar* f_dev, Scalar* g_dev, mi355_lbfgs_progress* progress_dev) const {
    Checked(Api::results(handle_, x_dev, f_dev, g_dev, progress_dev, stream_), "results");
  }
  // Listed mode (mi355_ask_tell_compact_*): rebuilds the list of the problems that have not finished and returns its
  // length.  From the first call on, row s < listed of Ask() is the point to evaluate for problem Ids()[s], and Tell /
  // TellAsync take f_dev [listed], g_dev [listed][n].  Waits for the stream.  Results() stays all B problems in order.
  int64_t Compact() {
    int64_t listed = 0;
    CheckedListed(Api::compact(handle_, &listed, stream_), "compact");
    return listed;
  }
  // DEVICE [listed()]: the numbers of the listed problems, ascending (valid until the next Compact()); nullptr before
  // the first Compact()
  const int64_t* Ids() const {
    const int64_t* p = nullptr;
    int64_t listed = 0;
    CheckedListed(Api::ids(handle_, &p, &listed), "ids");
    return p;
  }
  // the rows of Ask() / Tell(): the length of the list, batch() before the first Compact()
  int64_t listed() const {
    const int64_t* p = nullptr;
    int64_t listed = 0;
    CheckedListed(Api::ids(handle_, &p, &listed), "ids");
    return listed;
  }
  int64_t batch() const { return B_; }
  int dimension() const { return n_; }
  void* stream() const { return stream_; }

 protected:
  // create(ctx, &handle): the path's C create call, for a path whose create takes more than the common arguments
  template <class Create>
  AskTellHandle(std::shared_ptr<Context> context, int n, int64_t B, void* stream, Create create)
      : context_(std::move(context)), stream_(stream), B_(B), n_(n) {
    if (!context_) Fail(std::string(Api::kClass) + ": null context");
    Checked(create(context_->get(), &handle_), "create");
    Checked(Api::x(handle_, &x_), "x");
  }
  // Check() under the C function's full name, put together only when the call failed
  static void Checked(int rc, const char* function) {
    if (rc != MI355_OK) Check(rc, (std::string(Api::kPrefix) + function).c_str());
  }
  // ... for the calls of the listed mode, named mi355_ask_tell_<function>_<handle type>
  static void CheckedListed(int rc, const char* function) {
    if (rc != MI355_OK) Check(rc, (std::string("mi355_ask_tell_") + function + " (" + Api::kClass + ")").c_str());
  }

  std::shared_ptr<Context> context_;
  typename Api::Handle* handle_ = nullptr;
  const Scalar* x_ = nullptr;
  void* stream_ = nullptr;
  int64_t B_ = 0;
  int n_ = 0;
};

}  // namespace detail

class LbfgsAskTell : public detail::AskTellHandle<detail::LbfgsAskTellApi> {
 public:
  using AskTellHandle::AskTellHandle;
};

// ---- Lbfgs<F, m, MoreThuente> with ScalarType = float in the same form (mi355_lbfgs_ask_tell_f32_*) -----------------
// Every device array is float; the desc is AskTellDesc's (its thresholds are converted to float once by the library).
class LbfgsAskTellF32 : public detail::AskTellHandle<detail::LbfgsAskTellF32Api> {
 public:
  using AskTellHandle::AskTellHandle;
};

// ---- Lbfgsb<F, m, MoreThuente> in the same form (mi355_lbfgsb_ask_tell_*): simple bounds on the parameters -------------
// The fields of mi355_lbfgs_desc the path reads, with the reference's Lbfgsb defaults (m = 5, the default stopping
// progress with f_delta = 2.22e-9 relative, lbfgsb.h:84-87); the mapping is the library's.
inline mi355_lbfgs_desc LbfgsbAskTellDesc(int n, int m = 5, const mi355_lbfgs_stop* stop = nullptr) {
  mi355_lbfgs_desc d = {};
  d.objective = MI355_OBJ_ROSENBROCK;  // not read: the caller evaluates
  d.linesearch = MI355_LS_MORE_THUENTE;
  d.n = n;
  d.m = m;
  d.arithmetic = MI355_ARITH_EXACT;
  if (stop != nullptr) {
    d.stop = *stop;
  } else {
    Check(mi355_lbfgs_default_stop(2, &d.stop), "mi355_lbfgs_default_stop");
  }
  return d;
}

// How many problems asked for each kind of evaluation so far (LbfgsbAskTell::Asks); finished batch: the sum is the sum
// of nfev.
struct LbfgsbAsks {
  int64_t clip_start = 0, trial = 0, cauchy = 0, clip_next = 0, first = 0;
};

class LbfgsbAskTell : public detail::AskTellHandle<detail::LbfgsbAskTellApi> {
 public:
  // No box: the reference's default unbounded one.  x0_dev: DEVICE [B][n]; stream as for LbfgsAskTell.
  LbfgsbAskTell(std::shared_ptr<Context> context, const mi355_lbfgs_desc& desc, int64_t B, const double* x0_dev,
                void* stream = nullptr)
      : LbfgsbAskTell(std::move(context), desc, nullptr, nullptr, 0, B, x0_dev, stream) {}
  // One box shared by the batch: lower_dev / upper_dev are DEVICE arrays of n doubles.
  LbfgsbAskTell(std::shared_ptr<Context> context, const mi355_lbfgs_desc& desc, const double* lower_dev,
                const double* upper_dev, int64_t B, const double* x0_dev, void* stream = nullptr)
      : LbfgsbAskTell(std::move(context), desc, lower_dev, upper_dev, 0, B, x0_dev, stream) {}
  // One box per problem: DEVICE rows of box_stride >= n doubles.  The handle copies the box: the caller's may go.
  LbfgsbAskTell(std::shared_ptr<Context> context, const mi355_lbfgs_desc& desc, const double* lower_dev,
                const double* upper_dev, int64_t box_stride, int64_t B, const double* x0_dev, void* stream = nullptr)
      : AskTellHandle(std::move(context), desc.n, B, stream, [&](mi355_lbfgs_ctx* ctx, mi355_lbfgsb_ask_tell** out) {
          return mi355_lbfgsb_ask_tell_create(ctx, &desc, lower_dev, upper_dev, box_stride, B, x0_dev, stream, out);
        }) {}

  // waits for the stream
  LbfgsbAsks Asks() const {
    int64_t c[5] = {0, 0, 0, 0, 0};
    Checked(mi355_lbfgsb_ask_tell_asks(handle_, c, stream_), "asks");
    LbfgsbAsks a;
    a.clip_start = c[0];
    a.trial = c[1];
    a.cauchy = c[2];
    a.clip_next = c[3];
    a.first = c[4];
    return a;
  }
};

// The loop: evaluate, tell, until no problem is active.  f_dev [B] and g_dev [B][n] are the caller's work arrays; the
// evaluator must order its work on solve.stream().  max_rounds < 0: no limit; otherwise Fail() when the batch is still
// active after that many rounds.  Returns the number of rounds (= evaluations of the batch).
// Handle: LbfgsAskTell, LbfgsAskTellF32 or LbfgsbAskTell; the work arrays are of the handle's Scalar (double, float).
template <class Evaluator, class Handle>
int64_t MinimizeBatchWith(Evaluator&& evaluator, Handle& solve, typename Handle::Scalar* f_dev,
                          typename Handle::Scalar* g_dev, int64_t max_rounds = -1) {
  int64_t rounds = 0;
  if (solve.batch() == 0) return rounds;
  while (true) {
    evaluator(solve.Ask(), f_dev, g_dev, solve.batch(), solve.dimension());
    ++rounds;
    const int64_t active = solve.Tell(f_dev, g_dev);
    if (active == 0) return rounds;
    if (max_rounds >= 0 && rounds >= max_rounds)
      Fail("MinimizeBatchWith: " + std::to_string(active) + " problems still active after max_rounds = " +
           std::to_string(max_rounds) + " rounds");
  }
}

// The same loop over the LIST of the problems that have not finished, rebuilt every compact_every >= 1 rounds:
// evaluator(x_dev, f_dev, g_dev, rows, n, ids_dev) evaluates the `rows` listed problems only — x_dev [rows][n] their
// points, ids_dev [rows] their numbers (ascending, for per-problem data), f_dev [rows] and g_dev [rows][n] its output —
// so a finished problem costs no evaluation after the next compaction.  The work arrays hold B rows.  The active count
// is read every round and the loop ends with the batch: the number of rounds, and every bit of the results, are
// MinimizeBatchWith's.  Returns the number of rounds.
template <class Evaluator, class Handle>
int64_t MinimizeBatchWithCompaction(Evaluator&& evaluator, Handle& solve, typename Handle::Scalar* f_dev,
                                    typename Handle::Scalar* g_dev, int64_t compact_every = 1, int64_t max_rounds = -1) {
  if (compact_every < 1) Fail("MinimizeBatchWithCompaction: compact_every must be >= 1");
  int64_t rounds = 0;
  while (true) {
    const int64_t rows = solve.Compact();
    if (rows == 0) return rounds;
    const int64_t* const ids = solve.Ids();
    for (int64_t k = 0; k < compact_every; ++k) {
      evaluator(solve.Ask(), f_dev, g_dev, rows, solve.dimension(), ids);
      ++rounds;
      const int64_t active = solve.Tell(f_dev, g_dev);
      if (active == 0) return rounds;
      if (max_rounds >= 0 && rounds >= max_rounds)
        Fail("MinimizeBatchWithCompaction: " + std::to_string(active) + " problems still active after max_rounds = " +
             std::to_string(max_rounds) + " rounds");
    }
  }
}

// ... from the start points to the results, all DEVICE arrays (g_out / progress_out may be null).  x0_dev decides the
// precision: double arrays run LbfgsAskTell, float arrays LbfgsAskTellF32.
template <class Evaluator, class Scalar,
          class Solve = std::conditional_t<std::is_same<Scalar, float>::value, LbfgsAskTellF32, LbfgsAskTell>>
int64_t MinimizeBatchWith(Evaluator&& evaluator, std::shared_ptr<Context> context, const mi355_lbfgs_desc& desc, int64_t B,
                          const Scalar* x0_dev, typename Solve::Scalar* f_work_dev, typename Solve::Scalar* g_work_dev,
                          typename Solve::Scalar* x_out, typename Solve::Scalar* f_out, typename Solve::Scalar* g_out,
                          mi355_lbfgs_progress* progress_out, void* stream = nullptr, int64_t max_rounds = -1) {
  Solve solve(std::move(context), desc, B, x0_dev, stream);
  const int64_t rounds = MinimizeBatchWith(std::forward<Evaluator>(evaluator), solve, f_work_dev, g_work_dev, max_rounds);
  solve.Results(x_out, f_out, g_out, progress_out);
  return rounds;   // (the handle's destructor waits for the device: the results are in place)
}

}  // namespace cppoptlib::mi355
#endif  // CPPOPTLIB_MI355_ASK_TELL_H_
