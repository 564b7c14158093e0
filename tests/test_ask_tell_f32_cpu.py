"""The float ask/tell L-BFGS without a GPU: its symbols are declared, exported and listed; null arguments are argument
errors and crash nothing; LbfgsAskTellF32 compiles with plain g++ with and without exceptions; and the inputs of the
torch-objective GPU test are cleared on the float CPU twin (a condition on the inputs, not on the code under test)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import at32_lib
import l32_lib as L

REPO = os.path.dirname(at32_lib.HERE)
PROGRAM = os.path.join(at32_lib.HEADER_DIR, "atf_header_test.cc")


def test_symbols_are_declared_exported_and_listed():
    from cppnumericalsolvers_amd import capi
    lib = capi.load()
    header = open(os.path.join(REPO, "include", "mi355_lbfgs.h")).read()
    declared = set(re.findall(r"\b(mi355_lbfgs_ask_tell_f32_[a-z0-9_]+)\s*\(", header))
    assert declared == set(at32_lib.SYMBOLS)
    for name in at32_lib.SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.mi355_lbfgs_abi_version() == 9


def test_null_arguments_are_argument_errors():
    from cppnumericalsolvers_amd import capi
    lib = capi.load()
    d = capi.Desc()
    d.objective, d.linesearch, d.n, d.m = capi.OBJ_ROSENBROCK, capi.LS_MORE_THUENTE, 8, 6
    d.stop = capi.default_stop()
    h, p = C.c_void_p(), C.c_void_p()
    bad = capi.ERR_INVALID_ARGUMENT
    assert lib.mi355_lbfgs_ask_tell_f32_create(None, C.byref(d), 4, None, None, C.byref(h)) == bad
    assert "null context" in lib.mi355_lbfgs_last_error().decode() and not h.value
    assert lib.mi355_lbfgs_ask_tell_f32_create(None, C.byref(d), 4, None, None, None) == bad
    assert lib.mi355_lbfgs_ask_tell_f32_create(None, None, 4, None, None, C.byref(h)) == bad
    assert lib.mi355_lbfgs_ask_tell_f32_x(None, C.byref(p)) == bad
    assert lib.mi355_lbfgs_ask_tell_f32_step(None, None, None, None, None) == bad
    assert lib.mi355_lbfgs_ask_tell_f32_active(None, C.byref(p)) == bad
    assert lib.mi355_lbfgs_ask_tell_f32_results(None, None, None, None, None, None) == bad
    assert lib.mi355_lbfgs_ask_tell_f32_destroy(None) == 0


@pytest.mark.parametrize("flags", [(), ("-fno-exceptions",)], ids=["plain", "fno-exceptions"])
def test_header_program_compiles(flags):
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", *flags,
                          "-I" + os.path.join(REPO, "include"), PROGRAM], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "LbfgsAskTellF32" in open(PROGRAM).read()


def test_header_test_binaries_build():
    out = subprocess.run(["make", "-s", "-C", at32_lib.HEADER_DIR, "all"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for binary in ("atf_header_test", "atf_header_test_noexcept"):
        assert os.access(os.path.join(at32_lib.HEADER_DIR, "_build", binary), os.X_OK), binary


@pytest.mark.parametrize("halved", [True, False], ids=["centred_problem", "DiagQuadratic_a"])
def test_torch_objective_inputs_are_cleared_on_the_float_twin(halved):
    """The inputs of test_gpu_ask_tell_f32.py::test_value_only_torch_objective_in_float32 under their committed seed: the
    float twin in the reference's order, on the centred problem (DiagQuadratic(a / 2) from x0 - c, which is
    1/2 sum a_i x_i^2; and DiagQuadratic(a) as well), ends with the gradient status on all 131 starts at tau = 1e-4
    within the 200 iterations."""
    a, c, x0 = at32_lib.quadratic_inputs()
    assert a.dtype == c.dtype == x0.dtype == np.float32
    assert 0.5 <= a.min() and a.max() <= 2.0 and np.abs(c).max() <= 2.0 and np.abs(x0).max() <= 3.0
    coefficients = (a.astype(np.float64) / 2.0) if halved else a.astype(np.float64)
    stop = L.make_stop(**at32_lib.quadratic_stop_fields())
    x, f, g, p = L.twin_solve(L.DIAG_QUADRATIC, at32_lib.QUAD_M, x0 - c, params=np.concatenate([coefficients, [0.0]]),
                              stop=stop, order=L.REF_ORDER)
    print("float twin, %s: iterations <= %d, evaluations <= %d, gradient_norm <= %.3g"
          % ("a / 2" if halved else "a", p["num_iterations"].max(), p["nfev"].max(), p["gradient_norm"].max()))
    assert np.all(p["status"] == at32_lib.GRADIENT_STATUS), np.unique(p["status"], return_counts=True)
    assert p["gradient_norm"].max() <= at32_lib.QUAD_TAU
