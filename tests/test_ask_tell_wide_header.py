"""include/cppoptlib/mi355/ask_tell.h above n = 256: cppoptlib::mi355::LbfgsAskTell picks the workgroup-per-problem handle
(mi355_lbfgs_ask_tell_wide_*) by the dimension, and MinimizeBatchWith / MinimizeBatchWithCompaction follow.  Without a
GPU: the program over the header compiles with plain g++, with and without exceptions.  On the GPU: at n = 300, with the
library's evaluation as the callback, both loops return the persistent solve's bits."""
import os
import subprocess

import pytest

import atw_lib

REPO = os.path.dirname(atw_lib.HERE)
PROGRAM = os.path.join(atw_lib.TWIN_DIR, "atw_header_test.cc")


@pytest.mark.parametrize("flags", [(), ("-fno-exceptions",)], ids=["plain", "fno-exceptions"])
def test_header_program_compiles(flags):
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", *flags,
                          "-I" + os.path.join(REPO, "include"), PROGRAM], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    text = open(PROGRAM).read()
    assert "MinimizeBatchWith(" in text and "MinimizeBatchWithCompaction(" in text and "kN = 300" in text


def test_header_names_the_wide_handle():
    src = open(os.path.join(REPO, "include", "cppoptlib", "mi355", "ask_tell.h")).read()
    for name in ("create", "x", "step", "active", "results", "destroy", "compact", "ids"):
        assert "mi355_lbfgs_ask_tell_wide_" + name in src, name
    assert "desc->n > MI355_LBFGS_MAX_N" in src


@pytest.mark.gpu
def test_minimize_batch_with_at_n_300_is_the_persistent_solve():
    assert os.access(atw_lib.HEADER_TEST, os.X_OK), "%s is not built (run __graft_entry__.build())" % atw_lib.HEADER_TEST
    out = subprocess.run([atw_lib.HEADER_TEST], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    rounds = [int(line.split()[1]) for line in lines if line.startswith("rounds ")]
    assert len(rounds) == 2 and rounds[0] == rounds[1] and rounds[0] > 60   # (60 iterations, at least one trial each)
    rows = {tag: [line.split()[1:] for line in lines if line.startswith(tag + " ")]
            for tag in ("one_call", "compaction", "persistent")}
    assert len(rows["persistent"]) == 4 and all(len(r) == 2 * 300 + 19 for r in rows["persistent"]), out.stdout[:400]
    assert rows["one_call"] == rows["persistent"]
    assert rows["compaction"] == rows["persistent"]
    assert all(r[1] == "status" and r[2] in {"1", "2", "3", "4"} for r in rows["persistent"])   # ended on a stopping test
