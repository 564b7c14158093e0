// atc_header_test.cc — Compact(), Ids() and MinimizeBatchWithCompaction of include/cppoptlib/mi355/ask_tell.h, plain
// g++; the evaluator is a kernel of this test's own (atc_evaluator.hip, built by hipcc and linked in).
//   (no argument)  on the device: chained Rosenbrock, n = 5, m = 6, 37 starts of which every ninth is the minimiser (it
//                  finishes in its first round), under the parity stop with 200 iterations.  The evaluator sees the
//                  listed rows only and computes in the order of the library's functor, so the result must be the
//                  persistent kernel's bit for bit; prints one line per problem with every double as its bit pattern and
//                  the number of times the problem was evaluated, for tests/test_gpu_ask_tell_compact.py to hold against
//                  BatchedLbfgs.minimize.  Once with a compaction every round (tag k1), once every fourth (tag k4).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cppoptlib/mi355/ask_tell.h"

// the runtime calls this program needs, declared by hand: it is built by plain g++ without the HIP headers
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);  // 1: host to device, 2: device to host
int hipMemset(void* dst, int value, size_t size);
int hipDeviceSynchronize(void);
// atc_evaluator.hip
int atc_rosenbrock5(const double* x, double* f, double* g, long long rows, const long long* ids, unsigned* evaluations,
                    void* stream);
}

namespace amd = cppoptlib::mi355;

static unsigned long long bits(double v) {
  unsigned long long u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

static constexpr int kN = 5, kM = 6;
static constexpr int64_t kB = 37;

static mi355_lbfgs_stop parity_stop() {
  mi355_lbfgs_stop s;
  amd::Check(mi355_lbfgs_default_stop(0, &s), "mi355_lbfgs_default_stop");
  s.num_iterations = 200;
  s.x_delta = 1e-11;
  s.x_delta_violations = 1;
  s.f_delta = 0.0;
  s.gradient_norm = 1e-8;
  s.gradient_norm_relative = 1;
  s.past = 0;
  return s;
}

struct DeviceArrays {
  double *x0 = nullptr, *f = nullptr, *g = nullptr, *x_out = nullptr, *f_out = nullptr;
  mi355_lbfgs_progress* progress = nullptr;
  unsigned* evaluations = nullptr;
  DeviceArrays() {
    const size_t vec = sizeof(double) * kB * kN, sc = sizeof(double) * kB;
    bool ok = hipMalloc(reinterpret_cast<void**>(&x0), vec) == 0 && hipMalloc(reinterpret_cast<void**>(&f), sc) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&g), vec) == 0 && hipMalloc(reinterpret_cast<void**>(&x_out), vec) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&f_out), sc) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&progress), sizeof(mi355_lbfgs_progress) * kB) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&evaluations), sizeof(unsigned) * kB) == 0;
    if (!ok) amd::Fail("hipMalloc failed");
  }
  ~DeviceArrays() {
    for (void* p : {static_cast<void*>(x0), static_cast<void*>(f), static_cast<void*>(g), static_cast<void*>(x_out),
                    static_cast<void*>(f_out), static_cast<void*>(progress), static_cast<void*>(evaluations)})
      (void)hipFree(p);
  }
};

static int print_results(const char* tag, const DeviceArrays& d) {
  std::vector<double> x(kB * kN), f(kB);
  std::vector<mi355_lbfgs_progress> p(kB);
  std::vector<unsigned> evaluations(kB);
  if (hipDeviceSynchronize() != 0 || hipMemcpy(x.data(), d.x_out, sizeof(double) * x.size(), 2) != 0 ||
      hipMemcpy(f.data(), d.f_out, sizeof(double) * f.size(), 2) != 0 ||
      hipMemcpy(p.data(), d.progress, sizeof(mi355_lbfgs_progress) * p.size(), 2) != 0 ||
      hipMemcpy(evaluations.data(), d.evaluations, sizeof(unsigned) * evaluations.size(), 2) != 0) {
    std::printf("FAILED: copying the results back\n");
    return 1;
  }
  for (int64_t b = 0; b < kB; ++b) {
    std::printf("%s %" PRId64 " status %d iterations %u nfev %u evaluated %u f %016llx x", tag, b, p[b].status,
                p[b].num_iterations, p[b].nfev, evaluations[b], bits(f[b]));
    for (int j = 0; j < kN; ++j) std::printf(" %016llx", bits(x[b * kN + j]));
    std::printf("\n");
  }
  return 0;
}

static int on_device() {
  auto context = amd::Context::Default(0);
  const mi355_lbfgs_stop stop = parity_stop();
  const mi355_lbfgs_desc desc = amd::AskTellDesc(kN, kM, &stop);
  std::vector<double> x0(kB * kN);
  for (int64_t b = 0; b < kB; ++b)
    for (int j = 0; j < kN; ++j)
      x0[b * kN + j] = (b % 9 == 0) ? 1.0 : ((j % 2) ? 1.0 : -1.2) + 0.03125 * static_cast<double>(b);
  DeviceArrays d;
  if (hipMemcpy(d.x0, x0.data(), sizeof(double) * x0.size(), 1) != 0) amd::Fail("hipMemcpy failed");
  int64_t rows_seen = 0;
  auto evaluator = [&](const double* x_dev, double* f_dev, double* g_dev, int64_t rows, int n, const int64_t* ids_dev) {
    if (n != kN) amd::Fail("the evaluator is written for n = 5");
    static_assert(sizeof(long long) == sizeof(int64_t), "ids are handed on as long long");
    if (atc_rosenbrock5(x_dev, f_dev, g_dev, rows, reinterpret_cast<const long long*>(ids_dev), d.evaluations, nullptr) != 0)
      amd::Fail("the evaluator kernel failed to launch");
    rows_seen += rows;
  };
  int bad = 0;
  const int64_t every[2] = {1, 4};
  const char* const tags[2] = {"k1", "k4"};
  for (int run = 0; run < 2; ++run) {
    if (hipMemset(d.evaluations, 0, sizeof(unsigned) * kB) != 0) amd::Fail("hipMemset failed");
    rows_seen = 0;
    amd::LbfgsAskTell solve(context, desc, kB, d.x0);
    if (solve.Ids() != nullptr || solve.listed() != kB) amd::Fail("a handle is listed before its first Compact()");
    const int64_t rounds = amd::MinimizeBatchWithCompaction(evaluator, solve, d.f, d.g, every[run], 100000);
    if (solve.Compact() != 0 || solve.listed() != 0) amd::Fail("a finished batch lists something");
    solve.Results(d.x_out, d.f_out, nullptr, d.progress);
    std::printf("rounds %s %" PRId64 " rows %" PRId64 " of %" PRId64 "\n", tags[run], rounds, rows_seen, rounds * kB);
    bad |= print_results(tags[run], d);
  }
  return bad;
}

int main() { return on_device(); }
