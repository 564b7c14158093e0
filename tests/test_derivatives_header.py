"""include/cppoptlib/mi355/derivatives.h compiles with plain g++ -std=c++17, and with -fno-exceptions."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(REPO, "tests", "derivatives", "dv_header_test.cc")


@pytest.mark.parametrize("flags", [(), ("-fno-exceptions",)], ids=["plain", "no-exceptions"])
def test_header_compiles(tmp_path, flags):
    """The header test program uses every entry of the header: the four ...OnDevice functions and CheckDeviceTwin."""
    obj = str(tmp_path / "dv_header_test.o")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + os.path.join(REPO, "include"),
                           "-I" + os.path.join(REPO, "tests", "cpp"), "-I" + os.path.join(REPO, "tests", "derivatives"),
                           "-c", PROGRAM, "-o", obj])
    assert os.path.getsize(obj) > 0
