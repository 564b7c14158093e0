"""The drop-in headers include/cppoptlib/solver/gradient_descent.h and conjugated_gradient_descent.h on the CPU: they
compile with plain g++ -std=c++17, with -fno-exceptions too, need no linesearch/armijo.h of this project, refuse a
function type without derivatives at compile time with the reference's message, and GradientDescent refuses a line
search other than More-Thuente."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIRST = r'''
#include "cppoptlib/function.h"
#include "cppoptlib/solver/conjugated_gradient_descent.h"
#include "cppoptlib/solver/gradient_descent.h"
class Q : public cppoptlib::function::FunctionCRTP<Q, double, cppoptlib::function::DifferentiabilityMode::First> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* g = nullptr) const {
    if (g) { *g = VectorType(1); (*g)[0] = 2.0 * x[0]; }
    return x[0] * x[0];
  }
  auto DeviceTwin() const { return cppoptlib::mi355::twin::DiagQuadratic({1.0}, 0.0); }
};
template <class Solver>
int check() {
  Solver a;
  Solver b(cppoptlib::solver::DefaultStoppingSolverProgress<Q, typename Solver::StateType>());
  b.SetCallback([](const Q&, const typename Solver::StateType&, const typename Solver::ProgressType&) {});
  return (a.stopping_progress.num_iterations == b.stopping_progress.num_iterations) ? 0 : 1;
}
int main() {
  return check<cppoptlib::solver::GradientDescent<Q>>() +
         check<cppoptlib::solver::GradientDescent<Q, cppoptlib::solver::linesearch::MoreThuente>>() +
         check<cppoptlib::solver::ConjugatedGradientDescent<Q>>();
}
'''

VALUE_ONLY = r'''
#include "cppoptlib/function.h"
#include "cppoptlib/solver/%s.h"
class V : public cppoptlib::function::FunctionCRTP<V, double, cppoptlib::function::DifferentiabilityMode::None> {
 public:
  ScalarType operator()(const VectorType& x) const { return x[0] * x[0]; }
  auto DeviceTwin() const { return cppoptlib::mi355::twin::DiagQuadratic({1.0}, 0.0); }
};
int main() { cppoptlib::solver::%s<V> s; (void)s; }
'''

HAGER_ZHANG = r'''
#include "cppoptlib/function.h"
#include "cppoptlib/linesearch/hager_zhang.h"
#include "cppoptlib/solver/gradient_descent.h"
int main() {
  cppoptlib::solver::GradientDescent<cppoptlib::function::Rosenbrock<>, cppoptlib::solver::linesearch::HagerZhang> s;
  (void)s;
}
'''


def _compile(tmp_path, src, flags):
    p = tmp_path / "t.cc"
    p.write_text(src)
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(p)] + flags,
                          capture_output=True, text=True)


@pytest.mark.parametrize("flags", [[], ["-fno-exceptions"]], ids=["plain", "no-exceptions"])
def test_headers_compile(tmp_path, flags):
    r = _compile(tmp_path, FIRST, flags)
    assert r.returncode == 0, r.stderr


def test_headers_need_no_armijo_header():
    assert not os.path.exists(os.path.join(ROOT, "include", "cppoptlib", "linesearch", "armijo.h"))
    for name in ("gradient_descent.h", "conjugated_gradient_descent.h"):
        text = open(os.path.join(ROOT, "include", "cppoptlib", "solver", name)).read()
        assert "#include \"../linesearch/armijo" not in text
    text = open(os.path.join(ROOT, "include", "cppoptlib", "solver", "conjugated_gradient_descent.h")).read()
    assert "#include \"../linesearch" not in text


@pytest.mark.parametrize("header,solver", [("gradient_descent", "GradientDescent"),
                                           ("conjugated_gradient_descent", "ConjugatedGradientDescent")])
def test_function_without_derivatives_is_refused(tmp_path, header, solver):
    r = _compile(tmp_path, VALUE_ONLY % (header, solver), [])
    assert r.returncode != 0
    assert solver + " only supports first- or second-order" in r.stderr


def test_gradient_descent_refuses_hager_zhang(tmp_path):
    r = _compile(tmp_path, HAGER_ZHANG, [])
    assert r.returncode != 0
    assert "built for linesearch::MoreThuente only" in r.stderr
