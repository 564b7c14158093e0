"""Lbfgs<F, m>::SetNativeFloat of the C++ drop-in (include/cppoptlib/solver/lbfgs.h), without a GPU: the header test
compiles with plain g++ with and without -fno-exceptions (tests/lbfgs_f32/Makefile), and every misuse of the setter
fails through the existing Fail path with its message.  The solves of the same binary run in
tests/test_gpu_lbfgs_f32.py."""
import os
import subprocess

import l32_lib as L

BUILD = os.path.join(L.L32_DIR, "_build")


def _make():
    out = subprocess.run(["make", "-s", "-C", L.L32_DIR, "all"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_header_test_compiles_with_and_without_exceptions():
    _make()
    for name in ("f32_header_test", "f32_header_test_noexcept"):
        assert os.access(os.path.join(BUILD, name), os.X_OK), name


def test_misuse_fails_with_its_message():
    _make()
    out = subprocess.run([os.path.join(BUILD, "f32_header_test"), "--misuse"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == 5 and all(line.startswith("ok: ") for line in lines), out.stdout
    for what, text in (("double function", "ScalarType is not float"), ("Second-mode function", "First-mode functions"),
                       ("Hager-Zhang", "More-Thuente line search"), ("callback set before", "step callback"),
                       ("callback set after", "step callback")):
        assert any(line.startswith("ok: " + what) and text in line for line in lines), what


def test_float_program_without_the_setter_makes_the_calls_it_made_before():
    """The native entry is reached only behind the setter's flag: in the header every call of
    mi355_lbfgs_minimize_batch_f32_host sits in MinimizeBatchNativeFloat, which Minimize / MinimizeBatch enter only when
    native_float_ is set, and the flag is false unless SetNativeFloat(true) ran."""
    src = open(os.path.join(L.REPO, "include", "cppoptlib", "solver", "lbfgs.h")).read()
    assert src.count("mi355_lbfgs_minimize_batch_f32_host(") == 1
    assert src.count("if (native_float_) return MinimizeBatchNativeFloat(") == 2
    assert "bool native_float_ = false;" in src
    assert src.count("native_float_ = ") == 2   # the member's initialiser and the setter
