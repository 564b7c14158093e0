// cppoptlib/mi355/ask_tell.h — Lbfgs<F, m, MoreThuente> for an objective the CALLER evaluates on the device, without a
// device functor and without a second build of the library: reverse communication (ask / tell) over the C entry points
// mi355_lbfgs_ask_tell_* (include/mi355_lbfgs.h has the protocol).
//
//   LbfgsAskTell        RAII handle of one batched solve: Ask() is the device pointer of the points to evaluate
//                       ([B][n], the same pointer for the handle's lifetime), Tell(f_dev, g_dev) hands the values and
//                       gradients back and returns the number of problems still active, Results(...) copies the states.
//   LbfgsAskTellF32     the same in native float (mi355_lbfgs_ask_tell_f32_*): float x0, points, values, gradients and
//                       results — a float objective is evaluated in its own precision, never widened
//   LbfgsbAskTell       the same for Lbfgsb<F, m, MoreThuente>: no box, one shared box, or one box per problem
//                       (mi355_lbfgsb_ask_tell_*), plus Asks(), the count of every kind of evaluation asked for
//   MinimizeBatchWith   the loop around either: evaluator(x_dev, f_dev, g_dev, B, n) is the user's — its own kernels,
//                       hipBLAS, anything that leaves f [B] and g [B][n] in device memory, ordered on `stream`.
//
// Plain C++17: no HIP header is needed here; the device arrays are the caller's.  Failures surface through Fail()
// (context.h): an exception, or abort() when built with -fno-exceptions.
#ifndef CPPOPTLIB_MI355_ASK_TELL_H_
#define CPPOPTLIB_MI355_ASK_TELL_H_

#include <cstdint>
#include <memory>
#include <string>
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

class LbfgsAskTell {
 public:
  using Scalar = double;
  // x0_dev: DEVICE [B][n].  stream: a hipStream_t (nullptr: the default stream) for this and every later call.
  LbfgsAskTell(std::shared_ptr<Context> context, const mi355_lbfgs_desc& desc, int64_t B, const double* x0_dev,
               void* stream = nullptr)
      : context_(std::move(context)), stream_(stream), B_(B), n_(desc.n) {
    if (!context_) Fail("LbfgsAskTell: null context");
    Check(mi355_lbfgs_ask_tell_create(context_->get(), &desc, B, x0_dev, stream_, &handle_), "mi355_lbfgs_ask_tell_create");
    Check(mi355_lbfgs_ask_tell_x(handle_, &x_), "mi355_lbfgs_ask_tell_x");
  }
  ~LbfgsAskTell() { (void)mi355_lbfgs_ask_tell_destroy(handle_); }
  LbfgsAskTell(const LbfgsAskTell&) = delete;
  LbfgsAskTell& operator=(const LbfgsAskTell&) = delete;
  LbfgsAskTell(LbfgsAskTell&& other) noexcept
      : context_(std::move(other.context_)), handle_(other.handle_), x_(other.x_), stream_(other.stream_), B_(other.B_),
        n_(other.n_) {
    other.handle_ = nullptr;
  }
  LbfgsAskTell& operator=(LbfgsAskTell&&) = delete;

  // DEVICE [B][n]: the points to evaluate (rows of finished problems hold their returned x)
  const double* Ask() const { return x_; }
  // f_dev [B], g_dev [B][n]: the evaluation of Ask()'s rows.  Waits for the stream; returns the problems still active.
  int64_t Tell(const double* f_dev, const double* g_dev) {
    int64_t active = 0;
    Check(mi355_lbfgs_ask_tell_step(handle_, f_dev, g_dev, &active, stream_), "mi355_lbfgs_ask_tell_step");
    return active;
  }
  // ... without waiting: the count is behind ActiveDevice() once the stream has run the call
  void TellAsync(const double* f_dev, const double* g_dev) {
    Check(mi355_lbfgs_ask_tell_step(handle_, f_dev, g_dev, nullptr, stream_), "mi355_lbfgs_ask_tell_step");
  }
  const int64_t* ActiveDevice() const {
    const int64_t* p = nullptr;
    Check(mi355_lbfgs_ask_tell_active(handle_, &p), "mi355_lbfgs_ask_tell_active");
    return p;
  }
  // The current iterate of every problem, its value, gradient and progress record into DEVICE arrays (any may be null);
  // asynchronous on the stream.
  void Results(double* x_dev, double* f_dev, double* g_dev, mi355_lbfgs_progress* progress_dev) const {
    Check(mi355_lbfgs_ask_tell_results(handle_, x_dev, f_dev, g_dev, progress_dev, stream_), "mi355_lbfgs_ask_tell_results");
  }
  int64_t batch() const { return B_; }
  int dimension() const { return n_; }
  void* stream() const { return stream_; }

 private:
  std::shared_ptr<Context> context_;
  mi355_lbfgs_ask_tell* handle_ = nullptr;
  const double* x_ = nullptr;
  void* stream_ = nullptr;
  int64_t B_ = 0;
  int n_ = 0;
};

// ---- Lbfgs<F, m, MoreThuente> with ScalarType = float in the same form (mi355_lbfgs_ask_tell_f32_*) -----------------
// Every device array is float; the desc is AskTellDesc's (its thresholds are converted to float once by the library).
class LbfgsAskTellF32 {
 public:
  using Scalar = float;
  // x0_dev: DEVICE [B][n] floats.  stream: a hipStream_t (nullptr: the default stream) for this and every later call.
  LbfgsAskTellF32(std::shared_ptr<Context> context, const mi355_lbfgs_desc& desc, int64_t B, const float* x0_dev,
                  void* stream = nullptr)
      : context_(std::move(context)), stream_(stream), B_(B), n_(desc.n) {
    if (!context_) Fail("LbfgsAskTellF32: null context");
    Check(mi355_lbfgs_ask_tell_f32_create(context_->get(), &desc, B, x0_dev, stream_, &handle_),
          "mi355_lbfgs_ask_tell_f32_create");
    Check(mi355_lbfgs_ask_tell_f32_x(handle_, &x_), "mi355_lbfgs_ask_tell_f32_x");
  }
  ~LbfgsAskTellF32() { (void)mi355_lbfgs_ask_tell_f32_destroy(handle_); }
  LbfgsAskTellF32(const LbfgsAskTellF32&) = delete;
  LbfgsAskTellF32& operator=(const LbfgsAskTellF32&) = delete;
  LbfgsAskTellF32(LbfgsAskTellF32&& other) noexcept
      : context_(std::move(other.context_)), handle_(other.handle_), x_(other.x_), stream_(other.stream_), B_(other.B_),
        n_(other.n_) {
    other.handle_ = nullptr;
  }
  LbfgsAskTellF32& operator=(LbfgsAskTellF32&&) = delete;

  // DEVICE [B][n]: the points to evaluate (rows of finished problems hold their returned x)
  const float* Ask() const { return x_; }
  // f_dev [B], g_dev [B][n]: the evaluation of Ask()'s rows.  Waits for the stream; returns the problems still active.
  int64_t Tell(const float* f_dev, const float* g_dev) {
    int64_t active = 0;
    Check(mi355_lbfgs_ask_tell_f32_step(handle_, f_dev, g_dev, &active, stream_), "mi355_lbfgs_ask_tell_f32_step");
    return active;
  }
  // ... without waiting: the count is behind ActiveDevice() once the stream has run the call
  void TellAsync(const float* f_dev, const float* g_dev) {
    Check(mi355_lbfgs_ask_tell_f32_step(handle_, f_dev, g_dev, nullptr, stream_), "mi355_lbfgs_ask_tell_f32_step");
  }
  const int64_t* ActiveDevice() const {
    const int64_t* p = nullptr;
    Check(mi355_lbfgs_ask_tell_f32_active(handle_, &p), "mi355_lbfgs_ask_tell_f32_active");
    return p;
  }
  // The current iterate of every problem, its value, gradient and progress record into DEVICE arrays (any may be null);
  // asynchronous on the stream.
  void Results(float* x_dev, float* f_dev, float* g_dev, mi355_lbfgs_progress* progress_dev) const {
    Check(mi355_lbfgs_ask_tell_f32_results(handle_, x_dev, f_dev, g_dev, progress_dev, stream_),
          "mi355_lbfgs_ask_tell_f32_results");
  }
  int64_t batch() const { return B_; }
  int dimension() const { return n_; }
  void* stream() const { return stream_; }

 private:
  std::shared_ptr<Context> context_;
  mi355_lbfgs_ask_tell_f32* handle_ = nullptr;
  const float* x_ = nullptr;
  void* stream_ = nullptr;
  int64_t B_ = 0;
  int n_ = 0;
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

class LbfgsbAskTell {
 public:
  using Scalar = double;
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
      : context_(std::move(context)), stream_(stream), B_(B), n_(desc.n) {
    if (!context_) Fail("LbfgsbAskTell: null context");
    Check(mi355_lbfgsb_ask_tell_create(context_->get(), &desc, lower_dev, upper_dev, box_stride, B, x0_dev, stream_, &handle_),
          "mi355_lbfgsb_ask_tell_create");
    Check(mi355_lbfgsb_ask_tell_x(handle_, &x_), "mi355_lbfgsb_ask_tell_x");
  }
  ~LbfgsbAskTell() { (void)mi355_lbfgsb_ask_tell_destroy(handle_); }
  LbfgsbAskTell(const LbfgsbAskTell&) = delete;
  LbfgsbAskTell& operator=(const LbfgsbAskTell&) = delete;
  LbfgsbAskTell(LbfgsbAskTell&& other) noexcept
      : context_(std::move(other.context_)), handle_(other.handle_), x_(other.x_), stream_(other.stream_), B_(other.B_),
        n_(other.n_) {
    other.handle_ = nullptr;
  }
  LbfgsbAskTell& operator=(LbfgsbAskTell&&) = delete;

  const double* Ask() const { return x_; }
  int64_t Tell(const double* f_dev, const double* g_dev) {
    int64_t active = 0;
    Check(mi355_lbfgsb_ask_tell_step(handle_, f_dev, g_dev, &active, stream_), "mi355_lbfgsb_ask_tell_step");
    return active;
  }
  void TellAsync(const double* f_dev, const double* g_dev) {
    Check(mi355_lbfgsb_ask_tell_step(handle_, f_dev, g_dev, nullptr, stream_), "mi355_lbfgsb_ask_tell_step");
  }
  const int64_t* ActiveDevice() const {
    const int64_t* p = nullptr;
    Check(mi355_lbfgsb_ask_tell_active(handle_, &p), "mi355_lbfgsb_ask_tell_active");
    return p;
  }
  void Results(double* x_dev, double* f_dev, double* g_dev, mi355_lbfgs_progress* progress_dev) const {
    Check(mi355_lbfgsb_ask_tell_results(handle_, x_dev, f_dev, g_dev, progress_dev, stream_), "mi355_lbfgsb_ask_tell_results");
  }
  // waits for the stream
  LbfgsbAsks Asks() const {
    int64_t c[5] = {0, 0, 0, 0, 0};
    Check(mi355_lbfgsb_ask_tell_asks(handle_, c, stream_), "mi355_lbfgsb_ask_tell_asks");
    LbfgsbAsks a;
    a.clip_start = c[0];
    a.trial = c[1];
    a.cauchy = c[2];
    a.clip_next = c[3];
    a.first = c[4];
    return a;
  }
  int64_t batch() const { return B_; }
  int dimension() const { return n_; }
  void* stream() const { return stream_; }

 private:
  std::shared_ptr<Context> context_;
  mi355_lbfgsb_ask_tell* handle_ = nullptr;
  const double* x_ = nullptr;
  void* stream_ = nullptr;
  int64_t B_ = 0;
  int n_ = 0;
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

// ... from the start points to the results, all DEVICE arrays (g_out / progress_out may be null)
template <class Evaluator>
int64_t MinimizeBatchWith(Evaluator&& evaluator, std::shared_ptr<Context> context, const mi355_lbfgs_desc& desc, int64_t B,
                          const double* x0_dev, double* f_work_dev, double* g_work_dev, double* x_out, double* f_out,
                          double* g_out, mi355_lbfgs_progress* progress_out, void* stream = nullptr,
                          int64_t max_rounds = -1) {
  LbfgsAskTell solve(std::move(context), desc, B, x0_dev, stream);
  const int64_t rounds = MinimizeBatchWith(std::forward<Evaluator>(evaluator), solve, f_work_dev, g_work_dev, max_rounds);
  solve.Results(x_out, f_out, g_out, progress_out);
  return rounds;   // (the handle's destructor waits for the device: the results are in place)
}

// ... the same in native float (LbfgsAskTellF32)
template <class Evaluator>
int64_t MinimizeBatchWith(Evaluator&& evaluator, std::shared_ptr<Context> context, const mi355_lbfgs_desc& desc, int64_t B,
                          const float* x0_dev, float* f_work_dev, float* g_work_dev, float* x_out, float* f_out,
                          float* g_out, mi355_lbfgs_progress* progress_out, void* stream = nullptr,
                          int64_t max_rounds = -1) {
  LbfgsAskTellF32 solve(std::move(context), desc, B, x0_dev, stream);
  const int64_t rounds = MinimizeBatchWith(std::forward<Evaluator>(evaluator), solve, f_work_dev, g_work_dev, max_rounds);
  solve.Results(x_out, f_out, g_out, progress_out);
  return rounds;
}

}  // namespace cppoptlib::mi355
#endif  // CPPOPTLIB_MI355_ASK_TELL_H_
