"""The ask/tell L-BFGS-B without a GPU: its symbols are declared, exported and listed; null arguments are argument errors
and crash nothing; the header test program compiles with plain g++ with and without exceptions; the class is exported;
and the draw of the torch-objective GPU test is cleared on the CPU oracle (the reference algorithm alone lands within the
project's contract of the closed-form minimiser on every problem)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import at_lib
import atb_lib

REPO = os.path.dirname(atb_lib.HERE)
PROGRAM = os.path.join(atb_lib.BOX_DIR, "atb_header_test.cc")
NAMES = ["mi355_lbfgsb_ask_tell_" + s for s in ("create", "x", "step", "active", "results", "destroy", "asks")]


def test_symbols_are_declared_exported_and_listed():
    from cppnumericalsolvers_amd import capi
    lib = capi.load()
    header = open(os.path.join(REPO, "include", "mi355_lbfgs.h")).read()
    declared = set(re.findall(r"\b(mi355_lbfgsb_ask_tell_[a-z0-9_]+)\s*\(", header))
    assert declared == set(NAMES)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED_SYMBOLS, name
    assert lib.mi355_lbfgs_abi_version() == 9


def test_null_arguments_are_argument_errors():
    from cppnumericalsolvers_amd import capi
    lib = capi.load()
    d = capi.Desc()
    d.objective, d.linesearch, d.n, d.m = capi.OBJ_ROSENBROCK, capi.LS_MORE_THUENTE, 8, 5
    d.stop = capi.default_stop("lbfgsb")
    h, p = C.c_void_p(), C.c_void_p()
    counts = (C.c_int64 * 5)()
    bad = capi.ERR_INVALID_ARGUMENT
    assert lib.mi355_lbfgsb_ask_tell_create(None, C.byref(d), None, None, 0, 4, None, None, C.byref(h)) == bad
    assert "null context" in lib.mi355_lbfgs_last_error().decode() and not h.value
    assert lib.mi355_lbfgsb_ask_tell_create(None, C.byref(d), None, None, 0, 4, None, None, None) == bad
    assert lib.mi355_lbfgsb_ask_tell_create(None, None, None, None, 0, 4, None, None, C.byref(h)) == bad
    assert lib.mi355_lbfgsb_ask_tell_x(None, C.byref(p)) == bad
    assert lib.mi355_lbfgsb_ask_tell_step(None, None, None, None, None) == bad
    assert lib.mi355_lbfgsb_ask_tell_active(None, C.byref(p)) == bad
    assert lib.mi355_lbfgsb_ask_tell_results(None, None, None, None, None, None) == bad
    assert lib.mi355_lbfgsb_ask_tell_asks(None, counts, None) == bad
    assert lib.mi355_lbfgsb_ask_tell_destroy(None) == 0


def test_class_is_exported():
    import cppnumericalsolvers_amd as amd
    assert "LbfgsbAskTell" in amd.__all__ and issubclass(amd.LbfgsbAskTell, amd.LbfgsAskTell)
    assert amd.LbfgsbAskTell.ASK_KINDS == atb_lib.ASK_KINDS
    assert amd.BatchedLbfgsb.minimize_callable is amd.BatchedLbfgs.minimize_callable   # one driver loop for both


@pytest.mark.parametrize("flags", [(), ("-fno-exceptions",)], ids=["plain", "fno-exceptions"])
def test_header_program_compiles(flags):
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", *flags,
                          "-I" + os.path.join(REPO, "include"), PROGRAM], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_header_test_binaries_build():
    out = subprocess.run(["make", "-s", "-C", atb_lib.BOX_DIR, "all"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for binary in ("atb_header_test", "atb_header_test_noexcept"):
        assert os.access(os.path.join(atb_lib.BOX_DIR, "_build", binary), os.X_OK), binary


@pytest.mark.parametrize("n", atb_lib.TORCH_DIMS)
def test_torch_case_draw_is_within_the_contract_for_the_reference_algorithm(n):
    """the inputs of test_gpu_ask_tell_box.py::test_objective_written_in_torch_ops: the stop test reads the projected
    gradient of the iterate the last step started from, so |x - clip(c)| <= 1e-6 is no theorem; this draw is kept because
    the reference algorithm alone (the CPU oracle, DiagQuadratic in shifted coordinates) meets it on all 131 problems"""
    worst = atb_lib.torch_case_oracle_error(n)
    print("oracle, n = %d: max|x - clip(c)| = %.3g" % (n, worst))
    assert worst <= at_lib.CONTRACT
