// atb_header_test.cc — cppoptlib::mi355::LbfgsbAskTell and MinimizeBatchWith (include/cppoptlib/mi355/ask_tell.h), plain g++.
//   (no argument)  on the device: chained Rosenbrock, n = 13, m = 5, five starts (the last two outside the boxes), under the
//                  parity stop with 200 iterations, three times: no box, the shared box [-1.5, 0.8], and one box per
//                  problem (rows of stride 16: lower_b = -1.5 - b / 32, upper_b = 0.8 + b / 16).  The evaluator is the
//                  library's own evaluation entry (mi355_lbfgs_eval_batch), so each result must be the persistent
//                  reference-order kernel's bit for bit; prints one line per problem with every double as its bit pattern,
//                  for tests/test_gpu_ask_tell_box.py to hold against BatchedLbfgsb.minimize, and the ask counters.
//   --misuse       a refused desc fails through the Fail path with the library's text
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
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

static constexpr int kN = 13, kM = 5, kBoxStride = 16;
static constexpr int64_t kB = 5;

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
  double *x0 = nullptr, *f = nullptr, *g = nullptr, *x_out = nullptr, *f_out = nullptr, *g_out = nullptr;
  double *lower = nullptr, *upper = nullptr, *lower_rows = nullptr, *upper_rows = nullptr;
  mi355_lbfgs_progress* progress = nullptr;
  DeviceArrays() {
    const size_t vec = sizeof(double) * kB * kN, sc = sizeof(double) * kB, rows = sizeof(double) * kB * kBoxStride;
    bool ok = hipMalloc(reinterpret_cast<void**>(&x0), vec) == 0 && hipMalloc(reinterpret_cast<void**>(&f), sc) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&g), vec) == 0 && hipMalloc(reinterpret_cast<void**>(&x_out), vec) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&f_out), sc) == 0 && hipMalloc(reinterpret_cast<void**>(&g_out), vec) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&lower), sizeof(double) * kN) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&upper), sizeof(double) * kN) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&lower_rows), rows) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&upper_rows), rows) == 0 &&
              hipMalloc(reinterpret_cast<void**>(&progress), sizeof(mi355_lbfgs_progress) * kB) == 0;
    if (!ok) amd::Fail("hipMalloc failed");
  }
  ~DeviceArrays() {
    for (void* p : {static_cast<void*>(x0), static_cast<void*>(f), static_cast<void*>(g), static_cast<void*>(x_out),
                    static_cast<void*>(f_out), static_cast<void*>(g_out), static_cast<void*>(lower),
                    static_cast<void*>(upper), static_cast<void*>(lower_rows), static_cast<void*>(upper_rows),
                    static_cast<void*>(progress)})
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

template <class Evaluator>
static int run(const char* tag, Evaluator& evaluator, amd::LbfgsbAskTell solve, const DeviceArrays& d) {
  const int64_t rounds = amd::MinimizeBatchWith(evaluator, solve, d.f, d.g, 100000);
  solve.Results(d.x_out, d.f_out, d.g_out, d.progress);
  const amd::LbfgsbAsks a = solve.Asks();
  std::printf("rounds %s %" PRId64 " asks %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", tag, rounds,
              a.clip_start, a.trial, a.cauchy, a.clip_next, a.first);
  return print_results(tag, d);
}

static int on_device() {
  auto context = amd::Context::Default(0);
  const mi355_lbfgs_stop stop = parity_stop();
  const mi355_lbfgs_desc desc = amd::LbfgsbAskTellDesc(kN, kM, &stop);
  mi355_lbfgs_desc eval_desc = desc;  // the evaluation entry's desc: the library's mapping, exact arithmetic
  std::vector<double> x0(kB * kN), lo(kN, -1.5), hi(kN, 0.8), lo_rows(kB * kBoxStride, 0.0), hi_rows(kB * kBoxStride, 0.0);
  for (int64_t b = 0; b < kB; ++b) {
    for (int j = 0; j < kN; ++j) {
      x0[b * kN + j] = ((j % 2) ? 1.0 : -1.2) + 0.0625 * static_cast<double>(b) + (b >= 3 ? 1.0 : 0.0);
      lo_rows[b * kBoxStride + j] = -1.5 - static_cast<double>(b) / 32.0;
      hi_rows[b * kBoxStride + j] = 0.8 + static_cast<double>(b) / 16.0;
    }
  }
  DeviceArrays d;
  if (hipMemcpy(d.x0, x0.data(), sizeof(double) * x0.size(), 1) != 0 ||
      hipMemcpy(d.lower, lo.data(), sizeof(double) * kN, 1) != 0 || hipMemcpy(d.upper, hi.data(), sizeof(double) * kN, 1) != 0 ||
      hipMemcpy(d.lower_rows, lo_rows.data(), sizeof(double) * lo_rows.size(), 1) != 0 ||
      hipMemcpy(d.upper_rows, hi_rows.data(), sizeof(double) * hi_rows.size(), 1) != 0)
    amd::Fail("hipMemcpy failed");
  auto evaluator = [&](const double* x_dev, double* f_dev, double* g_dev, int64_t B, int n) {
    (void)n;
    amd::Check(mi355_lbfgs_eval_batch(context->get(), &eval_desc, B, x_dev, f_dev, g_dev, nullptr), "mi355_lbfgs_eval_batch");
  };
  int bad = 0;
  bad |= run("none", evaluator, amd::LbfgsbAskTell(context, desc, kB, d.x0), d);
  bad |= run("shared", evaluator, amd::LbfgsbAskTell(context, desc, d.lower, d.upper, kB, d.x0), d);
  bad |= run("rows", evaluator, amd::LbfgsbAskTell(context, desc, d.lower_rows, d.upper_rows, kBoxStride, kB, d.x0), d);
  return bad;
}

#if defined(__cpp_exceptions) || defined(__EXCEPTIONS)
static int misuse() {
  // (needs a context, hence a device: run with the GPU tests)
  auto context = amd::Context::Default(0);
  mi355_lbfgs_desc desc = amd::LbfgsbAskTellDesc(kN, kM);
  desc.linesearch = MI355_LS_HAGER_ZHANG;
  try {
    amd::LbfgsbAskTell solve(context, desc, kB, nullptr);
  } catch (const std::exception& e) {
    if (std::string(e.what()).find("Lbfgsb ask/tell") != std::string::npos &&
        std::string(e.what()).find("Hager-Zhang") != std::string::npos) {
      std::printf("ok: Hager-Zhang: %s\n", e.what());
      return 0;
    }
    std::printf("FAILED: another message: %s\n", e.what());
    return 1;
  }
  std::printf("FAILED: no failure\n");
  return 1;
}
#else
static int misuse() {
  std::printf("built without exceptions: a misuse ends the program (not run)\n");
  return 0;
}
#endif

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--misuse") == 0) return misuse();
  return on_device();
}
