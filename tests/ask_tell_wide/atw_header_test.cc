// atw_header_test.cc — cppoptlib::mi355::LbfgsAskTell and MinimizeBatchWith (include/cppoptlib/mi355/ask_tell.h) ABOVE
// n = 256, plain g++: the dimension picks the workgroup-per-problem handle (mi355_lbfgs_ask_tell_wide_*).
//   (no argument)  on the device: chained Rosenbrock, n = 300, m = 6, four starts, under the parity stop with 60
//                  iterations; the evaluator is the library's own evaluation entry (mi355_lbfgs_eval_batch), so the
//                  result must be the persistent kernel's (mi355_lbfgs_minimize_batch at the same n) bit for bit.  Prints
//                  one line per problem and solve with every double as its bit pattern — "one_call" through
//                  MinimizeBatchWith, "compaction" through MinimizeBatchWithCompaction, "persistent" through
//                  mi355_lbfgs_minimize_batch — for tests/test_ask_tell_wide_header.py to compare.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cppoptlib/mi355/ask_tell.h"

// the four runtime calls this program needs, declared by hand: it is built by plain g++ without the HIP headers
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);  // 1: host to device, 2: device to host
int hipDeviceSynchronize(void);
}

namespace amd = cppoptlib::mi355;

static unsigned long long bits(double v) {
  unsigned long long u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

static constexpr int kN = 300, kM = 6;
static constexpr int64_t kB = 4;

static mi355_lbfgs_stop parity_stop() {
  mi355_lbfgs_stop s;
  amd::Check(mi355_lbfgs_default_stop(0, &s), "mi355_lbfgs_default_stop");
  s.num_iterations = 60;
  s.x_delta = 1e-11;
  s.x_delta_violations = 1;
  s.f_delta = 0.0;
  s.gradient_norm = 1e-8;
  s.gradient_norm_relative = 1;
  s.past = 0;
  return s;
}

struct DeviceArrays {
  double *x0 = nullptr, *f = nullptr, *g = nullptr, *x_out = nullptr, *f_out = nullptr, *g_out = nullptr;
  mi355_lbfgs_progress* progress = nullptr;
  DeviceArrays() {
    const size_t vec = sizeof(double) * kB * kN, sc = sizeof(double) * kB;
    bool ok = hipMalloc(reinterpret_cast<void**>(&x0), vec) == 0 && hipMalloc(reinterpret_cast<void**>(&f), sc) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&g), vec) == 0 && hipMalloc(reinterpret_cast<void**>(&x_out), vec) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&f_out), sc) == 0 && hipMalloc(reinterpret_cast<void**>(&g_out), vec) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&progress), sizeof(mi355_lbfgs_progress) * kB) == 0;
    if (!ok) amd::Fail("hipMalloc failed");
  }
  ~DeviceArrays() {
    for (void* p : {static_cast<void*>(x0), static_cast<void*>(f), static_cast<void*>(g), static_cast<void*>(x_out),
                    static_cast<void*>(f_out), static_cast<void*>(g_out), static_cast<void*>(progress)})
      (void)hipFree(p);
  }
};

static int print_results(const char* tag, const DeviceArrays& d) {
  std::vector<double> x(kB * kN), g(kB * kN), f(kB);
  std::vector<mi355_lbfgs_progress> p(kB);
  if (hipDeviceSynchronize() != 0 || hipMemcpy(x.data(), d.x_out, sizeof(double) * x.size(), 2) != 0 ||
      hipMemcpy(g.data(), d.g_out, sizeof(double) * g.size(), 2) != 0 ||
      hipMemcpy(f.data(), d.f_out, sizeof(double) * f.size(), 2) != 0 ||
      hipMemcpy(p.data(), d.progress, sizeof(mi355_lbfgs_progress) * p.size(), 2) != 0) {
    std::printf("FAILED: copying the results back\n");
    return 1;
  }
  for (int64_t b = 0; b < kB; ++b) {
    std::printf("%s %" PRId64 " status %d iterations %u nfev %u sum_k %u x_delta %016llx f_delta %016llx gradient_norm %016llx f %016llx x",
                tag, b, p[b].status, p[b].num_iterations, p[b].nfev, p[b].sum_k, bits(p[b].x_delta), bits(p[b].f_delta),
                bits(p[b].gradient_norm), bits(f[b]));
    for (int j = 0; j < kN; ++j) std::printf(" %016llx", bits(x[b * kN + j]));
    std::printf(" g");
    for (int j = 0; j < kN; ++j) std::printf(" %016llx", bits(g[b * kN + j]));
    std::printf("\n");
  }
  return 0;
}

int main() {
  auto context = amd::Context::Default(0);
  const mi355_lbfgs_stop stop = parity_stop();
  const mi355_lbfgs_desc desc = amd::AskTellDesc(kN, kM, &stop);
  mi355_lbfgs_desc eval_desc = desc;  // the evaluation entry's: Rosenbrock, the library's mapping, exact arithmetic
  std::vector<double> x0(kB * kN);
  for (int64_t b = 0; b < kB; ++b)
    for (int j = 0; j < kN; ++j) x0[b * kN + j] = ((j % 2) ? 1.0 : -1.2) + 0.0625 * static_cast<double>(b);
  DeviceArrays d;
  if (hipMemcpy(d.x0, x0.data(), sizeof(double) * x0.size(), 1) != 0) amd::Fail("hipMemcpy failed");
  auto evaluator = [&](const double* x_dev, double* f_dev, double* g_dev, int64_t B, int n, const int64_t* = nullptr) {
    (void)n;
    amd::Check(mi355_lbfgs_eval_batch(context->get(), &eval_desc, B, x_dev, f_dev, g_dev, nullptr), "mi355_lbfgs_eval_batch");
  };
  int bad = 0;
  {
    const int64_t rounds = amd::MinimizeBatchWith(evaluator, context, desc, kB, d.x0, d.f, d.g, d.x_out, d.f_out, d.g_out,
                                                  d.progress);
    std::printf("rounds %" PRId64 "\n", rounds);
    bad |= print_results("one_call", d);
  }
  {
    amd::LbfgsAskTell solve(context, desc, kB, d.x0);
    const int64_t rounds = amd::MinimizeBatchWithCompaction(evaluator, solve, d.f, d.g, 2);
    solve.Results(d.x_out, d.f_out, d.g_out, d.progress);
    std::printf("rounds %" PRId64 "\n", rounds);
    bad |= print_results("compaction", d);
  }
  {
    amd::Check(mi355_lbfgs_minimize_batch(context->get(), &eval_desc, kB, d.x0, d.x_out, d.f_out, d.g_out, d.progress, nullptr),
               "mi355_lbfgs_minimize_batch");
    bad |= print_results("persistent", d);
  }
  return bad;
}
