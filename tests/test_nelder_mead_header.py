"""The drop-in header include/cppoptlib/solver/nelder_mead.h on the CPU: it compiles with plain g++ -std=c++17 (with
-fno-exceptions too) for None-, First- and Second-mode function types, and the default constructor yields the
conservative stopping preset with five x_delta strikes, as the reference's does (the prebuilt header test's --preset
part, which touches no device)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r'''
#include "cppoptlib/function.h"
#include "cppoptlib/solver/nelder_mead.h"
using cppoptlib::function::DifferentiabilityMode;
class V : public cppoptlib::function::FunctionCRTP<V, double, DifferentiabilityMode::None> {
 public:
  ScalarType operator()(const VectorType& x) const { return x[0] * x[0]; }
  auto DeviceTwin() const { return cppoptlib::mi355::twin::DiagQuadratic({1.0}, 0.0); }
};
class Q : public cppoptlib::function::FunctionCRTP<Q, double, DifferentiabilityMode::Second> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* g = nullptr, MatrixType* h = nullptr) const {
    if (g) { *g = VectorType(1); (*g)[0] = 2.0 * x[0]; }
    if (h) { *h = MatrixType(1, 1); (*h)(0, 0) = 2.0; }
    return x[0] * x[0];
  }
  auto DeviceTwin() const { return cppoptlib::mi355::twin::DiagQuadratic({1.0}, 0.0); }
};
int main() {
  cppoptlib::solver::NelderMead<V> s;
  cppoptlib::solver::NelderMead<Q> q;
  cppoptlib::solver::NelderMead<cppoptlib::function::Rosenbrock<>> r;
  s.SetCallback([](const V&, const auto&, const auto&) {});
  return (s.stopping_progress.x_delta_violations == 5 && q.stopping_progress.past == 5 &&
          r.stopping_progress.x_delta_violations == 5) ? 0 : 1;
}
'''


@pytest.mark.parametrize("flags", [[], ["-fno-exceptions"]], ids=["plain", "no-exceptions"])
def test_header_compiles(tmp_path, flags):
    p = tmp_path / "t.cc"
    p.write_text(SOURCE)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), str(p)] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_constructor_yields_the_conservative_preset_with_five_strikes():
    exe = os.path.join(ROOT, "tests", "nelder_mead", "_build", "nm_header_test")
    r = subprocess.run([exe, "--preset"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
