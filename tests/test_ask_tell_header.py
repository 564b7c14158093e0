"""include/cppoptlib/mi355/ask_tell.h and the ask/tell twin's sanitizer build, without a GPU: a program over the header
compiles with plain g++ with and without -fno-exceptions, and the twin's stand-alone `make sanitize` run (address and
undefined-behaviour sanitizers) is clean.  The header test binary's solves run in tests/test_gpu_ask_tell.py."""
import os
import subprocess

import pytest

import at_lib

REPO = os.path.dirname(at_lib.HERE)
PROGRAM = os.path.join(at_lib.TWIN_DIR, "at_header_test.cc")


@pytest.mark.parametrize("flags", [(), ("-fno-exceptions",)], ids=["plain", "fno-exceptions"])
def test_header_program_compiles(flags):
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", *flags,
                          "-I" + os.path.join(REPO, "include"), PROGRAM], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_header_needs_no_hip_header():
    """plain g++: the header includes the C ABI and the standard library only"""
    src = open(os.path.join(REPO, "include", "cppoptlib", "mi355", "ask_tell.h")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert all(not inc.strip('<>"').startswith("hip") for inc in includes), includes
    assert '"context.h"' in includes


def test_sanitize_target_runs_clean():
    out = subprocess.run(["make", "-s", "-C", at_lib.TWIN_DIR, "sanitize"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert out.stdout.count("status") == 18   # three cases, two orders, three problems
