// atf_header_test.cc — cppoptlib::mi355::LbfgsAskTellF32 and the float MinimizeBatchWith
// (include/cppoptlib/mi355/ask_tell.h), plain g++.
//   (no argument)  on the device: chained Rosenbrock in float, n = 13, m = 6, five starts (x0[b][j] = -1.25 or 1 by the
//                  parity of j, plus b / 16: exact in float), under the reference's default stop.  The evaluator is the
//                  library's own float evaluation entry (mi355_lbfgs_eval_batch_f32), so the result must be the
//                  persistent float kernel's bit for bit; prints one line per problem with every float and every double
//                  as its bit pattern, for tests/test_gpu_ask_tell_f32.py to hold against
//                  BatchedLbfgs(dtype=torch.float32).minimize.  Once through the handle (Tell), once through the
//                  one-call overload.
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
static unsigned bits(float v) {
  unsigned u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

static constexpr int kN = 13, kM = 6;
static constexpr int64_t kB = 5;

struct DeviceArrays {
  float *x0 = nullptr, *f = nullptr, *g = nullptr, *x_out = nullptr, *f_out = nullptr, *g_out = nullptr;
  mi355_lbfgs_progress* progress = nullptr;
  DeviceArrays() {
    const size_t vec = sizeof(float) * kB * kN, sc = sizeof(float) * kB;
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
  std::vector<float> x(kB * kN), g(kB * kN), f(kB);
  std::vector<mi355_lbfgs_progress> p(kB);
  if (hipDeviceSynchronize() != 0 || hipMemcpy(x.data(), d.x_out, sizeof(float) * x.size(), 2) != 0 ||
      hipMemcpy(g.data(), d.g_out, sizeof(float) * g.size(), 2) != 0 ||
      hipMemcpy(f.data(), d.f_out, sizeof(float) * f.size(), 2) != 0 ||
      hipMemcpy(p.data(), d.progress, sizeof(mi355_lbfgs_progress) * p.size(), 2) != 0) {
    std::printf("FAILED: copying the results back\n");
    return 1;
  }
  for (int64_t b = 0; b < kB; ++b) {
    std::printf("%s %" PRId64 " status %d iterations %u nfev %u sum_k %u x_delta %016llx f_delta %016llx gradient_norm %016llx f %08x x",
                tag, b, p[b].status, p[b].num_iterations, p[b].nfev, p[b].sum_k, bits(p[b].x_delta), bits(p[b].f_delta),
                bits(p[b].gradient_norm), bits(f[b]));
    for (int j = 0; j < kN; ++j) std::printf(" %08x", bits(x[b * kN + j]));
    std::printf(" g");
    for (int j = 0; j < kN; ++j) std::printf(" %08x", bits(g[b * kN + j]));
    std::printf("\n");
  }
  return 0;
}

static int on_device() {
  auto context = amd::Context::Default(0);
  const mi355_lbfgs_desc desc = amd::AskTellDesc(kN, kM);
  mi355_lbfgs_desc eval_desc = desc;  // the evaluation entry's desc: Rosenbrock, the library's mapping, exact arithmetic
  std::vector<float> x0(kB * kN);
  for (int64_t b = 0; b < kB; ++b)
    for (int j = 0; j < kN; ++j) x0[b * kN + j] = ((j % 2) ? 1.0f : -1.25f) + 0.0625f * static_cast<float>(b);
  DeviceArrays d;
  if (hipMemcpy(d.x0, x0.data(), sizeof(float) * x0.size(), 1) != 0) amd::Fail("hipMemcpy failed");
  auto evaluator = [&](const float* x_dev, float* f_dev, float* g_dev, int64_t B, int n) {
    (void)n;
    amd::Check(mi355_lbfgs_eval_batch_f32(context->get(), &eval_desc, B, x_dev, f_dev, g_dev, nullptr),
               "mi355_lbfgs_eval_batch_f32");
  };
  int bad = 0;
  {
    amd::LbfgsAskTellF32 solve(context, desc, kB, d.x0);
    const int64_t rounds = amd::MinimizeBatchWith(evaluator, solve, d.f, d.g, 100000);
    solve.Results(d.x_out, d.f_out, d.g_out, d.progress);
    std::printf("rounds handle %" PRId64 "\n", rounds);
    bad |= print_results("handle", d);
  }
  {
    const int64_t rounds = amd::MinimizeBatchWith(evaluator, context, desc, kB, d.x0, d.f, d.g, d.x_out, d.f_out, d.g_out,
                                                  d.progress, nullptr, 100000);
    std::printf("rounds call %" PRId64 "\n", rounds);
    bad |= print_results("call", d);
  }
  return bad;
}

#if defined(__cpp_exceptions) || defined(__EXCEPTIONS)
static int misuse() {
  // (needs a context, hence a device: run with the GPU tests)
  auto context = amd::Context::Default(0);
  mi355_lbfgs_desc desc = amd::AskTellDesc(kN, kM);
  desc.linesearch = MI355_LS_HAGER_ZHANG;
  try {
    amd::LbfgsAskTellF32 solve(context, desc, kB, nullptr);
  } catch (const std::exception& e) {
    if (std::string(e.what()).find("Lbfgs ask/tell f32") != std::string::npos &&
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
