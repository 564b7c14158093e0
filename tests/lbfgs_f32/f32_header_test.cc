// f32_header_test.cc — Lbfgs<F, m>::SetNativeFloat over the drop-in headers (include/cppoptlib/solver/lbfgs.h), plain g++.
//   (no argument)  on the device: the 2-D Rosenbrock of the reference's verify.cc as a FLOAT function from its two starts,
//                  through Minimize and through MinimizeBatch with the native fp32 kernel, and once without the setter
//                  (the widened fp64 path); prints one line per result with every float as its bit pattern, for
//                  tests/test_gpu_lbfgs_f32.py to hold against the CPU twin
//   --misuse       without a device: every misuse of the setter fails through the Fail path with its message
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cppoptlib/function.h"
#include "cppoptlib/linesearch/hager_zhang.h"
#include "cppoptlib/solver/lbfgs.h"

using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;
using cppoptlib::function::FunctionState;
using cppoptlib::solver::Lbfgs;
namespace twin = cppoptlib::mi355::twin;

template <class T, DifferentiabilityMode Mode>
class RosenbrockT : public FunctionCRTP<RosenbrockT<T, Mode>, T, Mode> {
 public:
  using Base = FunctionCRTP<RosenbrockT<T, Mode>, T, Mode>;
  using typename Base::MatrixType;
  using typename Base::ScalarType;
  using typename Base::VectorType;
  ScalarType operator()(const VectorType& x, VectorType* grad = nullptr, MatrixType* = nullptr) const {
    const T t1 = 1 - x[0];
    const T t2 = x[1] - x[0] * x[0];
    if (grad) {
      *grad = VectorType(2);
      (*grad)[0] = -2 * t1 + 200 * t2 * (-2 * x[0]);
      (*grad)[1] = 200 * t2;
    }
    return t1 * t1 + 100 * t2 * t2;
  }
  auto DeviceTwin() const { return twin::Rosenbrock(); }
};
using RosenbrockF = RosenbrockT<float, DifferentiabilityMode::First>;
using RosenbrockD = RosenbrockT<double, DifferentiabilityMode::First>;

static RosenbrockF::VectorType vec(float a, float b) {
  RosenbrockF::VectorType v(2);
  v[0] = a;
  v[1] = b;
  return v;
}
static unsigned bits(float v) {
  unsigned u;
  std::memcpy(&u, &v, sizeof u);
  return u;
}

template <class State, class Progress>
static void print(const char* tag, const State& s, const Progress& p) {
  std::printf("%s x %08x %08x f %08x g %08x %08x status %d iterations %u x_delta %08x f_delta %08x gradient_norm %08x\n", tag,
              bits(s.x[0]), bits(s.x[1]), bits(s.value), bits(s.gradient[0]), bits(s.gradient[1]), static_cast<int>(p.status),
              static_cast<unsigned>(p.num_iterations), bits(p.x_delta), bits(p.f_delta), bits(p.gradient_norm));
}

static int on_device() {
  RosenbrockF f;
  const float starts[2][2] = {{15.0f, 8.0f}, {-1.0f, 2.0f}};
  std::vector<Lbfgs<RosenbrockF, 6>::StateType> states;
  for (const auto& s : starts) {
    Lbfgs<RosenbrockF, 6> solver;
    solver.SetNativeFloat(true);
    auto [solution, progress] = solver.Minimize(f, FunctionState(vec(s[0], s[1])));
    print("minimize", solution, progress);
    states.emplace_back(vec(s[0], s[1]));
  }
  Lbfgs<RosenbrockF, 6> batch;
  batch.SetNativeFloat(true);
  for (const auto& r : batch.MinimizeBatch(f, states)) print("batch", std::get<0>(r), std::get<1>(r));
  Lbfgs<RosenbrockF, 6> widened;   // the setter not called: the fp64 engine, results rounded to float
  widened.SetArithmetic(MI355_ARITH_EXACT);
  for (const auto& r : widened.MinimizeBatch(f, states)) print("widened", std::get<0>(r), std::get<1>(r));
  return 0;
}

#if defined(__cpp_exceptions) || defined(__EXCEPTIONS)
template <class Call>
static int fails_with(const char* what, const char* text, Call call) {
  try {
    call();
  } catch (const std::exception& e) {
    if (std::string(e.what()).find(text) != std::string::npos) {
      std::printf("ok: %s: %s\n", what, e.what());
      return 0;
    }
    std::printf("FAILED: %s: another message: %s\n", what, e.what());
    return 1;
  }
  std::printf("FAILED: %s: no failure\n", what);
  return 1;
}

static int misuse() {
  int bad = 0;
  bad += fails_with("double function", "ScalarType is not float", [] {
    Lbfgs<RosenbrockD, 6> s;
    s.SetNativeFloat(true);
  });
  bad += fails_with("Second-mode function", "First-mode functions", [] {
    Lbfgs<RosenbrockT<float, DifferentiabilityMode::Second>, 6> s;
    s.SetNativeFloat(true);
  });
  bad += fails_with("Hager-Zhang", "More-Thuente line search", [] {
    Lbfgs<RosenbrockF, 6, cppoptlib::solver::linesearch::HagerZhang> s;
    s.SetNativeFloat(true);
  });
  bad += fails_with("callback set before", "step callback", [] {
    Lbfgs<RosenbrockF, 6> s;
    s.SetCallback([](const RosenbrockF&, const auto&, const auto&) {});
    s.SetNativeFloat(true);
  });
  bad += fails_with("callback set after", "step callback", [] {
    Lbfgs<RosenbrockF, 6> s;
    s.SetNativeFloat(true);
    s.SetCallback([](const RosenbrockF&, const auto&, const auto&) {});
    RosenbrockF f;
    s.Minimize(f, FunctionState(vec(-1.0f, 2.0f)));
  });
  {  // off by default, and switching it off again is always allowed
    Lbfgs<RosenbrockF, 6> s;
    Lbfgs<RosenbrockD, 6> d;
    d.SetNativeFloat(false);
    if (s.NativeFloat() || d.NativeFloat()) {
      std::printf("FAILED: the native path is not off by default\n");
      ++bad;
    }
  }
  return bad;
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
