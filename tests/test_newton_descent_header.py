"""The drop-in header include/cppoptlib/solver/newton_descent.h on the CPU: it compiles with plain g++ -std=c++17, with
-fno-exceptions too, needs no linesearch/armijo.h of this project, and refuses a First-mode function type at compile
time with the reference's message."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SECOND = r'''
#include "cppoptlib/function.h"
#include "cppoptlib/solver/newton_descent.h"
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
  using Solver = cppoptlib::solver::NewtonDescent<Q>;
  Solver a;
  Solver b(cppoptlib::solver::DefaultStoppingSolverProgress<Q, Solver::StateType>());
  b.SetCallback([](const Q&, const Solver::StateType&, const Solver::ProgressType&) {});
  return (a.stopping_progress.num_iterations == b.stopping_progress.num_iterations) ? 0 : 1;
}
'''

FIRST = r'''
#include "cppoptlib/function.h"
#include "cppoptlib/solver/newton_descent.h"
int main() { cppoptlib::solver::NewtonDescent<cppoptlib::function::Rosenbrock<>> s; (void)s; }
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


def test_header_needs_no_armijo_header():
    assert not os.path.exists(os.path.join(ROOT, "include", "cppoptlib", "linesearch", "armijo.h"))
    text = open(os.path.join(ROOT, "include", "cppoptlib", "solver", "newton_descent.h")).read()
    assert "#include \"../linesearch" not in text


def test_first_mode_function_is_refused(tmp_path):
    r = _compile(tmp_path, FIRST, [])
    assert r.returncode != 0
    assert "NewtonDescent only supports second-order" in r.stderr
