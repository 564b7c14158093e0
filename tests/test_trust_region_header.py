"""The drop-in header include/cppoptlib/solver/trust_region_newton.h on the CPU: it compiles with plain g++ -std=c++17, with
-fno-exceptions too, and refuses a First-mode function type at compile time, as the reference does."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SECOND = r'''
#include "cppoptlib/function.h"
#include "cppoptlib/solver/trust_region_newton.h"
class Q : public cppoptlib::function::FunctionCRTP<Q, double, cppoptlib::function::DifferentiabilityMode::Second> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* g = nullptr, MatrixType* h = nullptr) const {
    if (g) { *g = VectorType(1); (*g)[0] = 2.0 * x[0]; }
    if (h) { *h = MatrixType(1, 1); (*h)(0, 0) = 2.0; }
    return x[0] * x[0];
  }
  auto DeviceTwin() const { return cppoptlib::mi355::twin::DiagQuadratic({1.0}, 0.0); }
};
int main() {
  cppoptlib::solver::TrustRegionNewtonConfig<double> c;
  cppoptlib::solver::TrustRegionNewton<Q> s(c);
  return (s.config().initial_radius == 1.0 && s.config().rejection_retry_limit == 50 &&
          s.config().cg_max_iterations_floor == 10) ? 0 : 1;
}
'''

FIRST = r'''
#include "cppoptlib/function.h"
#include "cppoptlib/solver/trust_region_newton.h"
int main() { cppoptlib::solver::TrustRegionNewton<cppoptlib::function::Rosenbrock<>> s; (void)s; }
'''


def _compile(tmp_path, src, flags):
    p = tmp_path / "t.cc"
    p.write_text(src)
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(p)] + flags,
                          capture_output=True, text=True)


@pytest.mark.parametrize("flags", [[], ["-fno-exceptions"]], ids=["plain", "no-exceptions"])
def test_header_compiles(tmp_path, flags):
    r = _compile(tmp_path, SECOND, flags)
    assert r.returncode == 0, r.stderr


def test_first_mode_function_is_refused(tmp_path):
    r = _compile(tmp_path, FIRST, [])
    assert r.returncode != 0
    assert "requires second-order differentiability" in r.stderr
