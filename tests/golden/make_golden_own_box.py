"""Writes tests/golden/own_box_reference_n40_m7.npz: the reference's own Lbfgsb<F, 7> (its solver/lbfgsb.h over the Eigen
stand-in, tests/own_box/ref_harness.cpp compiled into a temporary directory outside the tree) on the case exact_n40_m7 of
tests/own_box_cases.py, every row under SetBounds with that row's box, parity stopping.  The reference binary of
oracle/_ref holds no history size 7 on the Rosenbrock function; the other exact cases are compared with it directly.
Run by hand where the reference tree exists, after build():
    python tests/golden/make_golden_own_box.py

The file holds the reference's x, f, status and num_iterations and a SHA-256 digest of the inputs (x0, lower, upper), so
that a test cannot compare against results of other inputs."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
import oracle_lib  # noqa: E402
import own_box_cases as cases  # noqa: E402

OUT = os.path.join(HERE, "own_box_reference_n40_m7.npz")
REFERENCE = "/root/reference"


def main():
    case = cases.BY_NAME["exact_n40_m7"]
    x0, lower, upper, _ = cases.inputs(case)
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "libown_box_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                               "-I" + os.path.join(os.path.dirname(TESTS), "oracle", "eigen_shim"),
                               "-I" + os.path.join(REFERENCE, "include"),
                               os.path.join(TESTS, "own_box", "ref_harness.cpp"), "-o", lib])
        L = C.CDLL(lib)
        x, f = np.empty_like(x0), np.empty(cases.B)
        status, iterations = np.zeros(cases.B, dtype=np.int32), np.zeros(cases.B, dtype=np.uint32)
        stop = oracle_lib.parity_stop()
        L.own_box_ref_rosenbrock_m7.argtypes = [C.c_int, C.c_int64, C.c_void_p] + [C.c_void_p] * 7
        rc = L.own_box_ref_rosenbrock_m7(case["n"], cases.B, C.addressof(stop), lower.ctypes.data, upper.ctypes.data,
                                         x0.ctypes.data, x.ctypes.data, f.ctypes.data, status.ctypes.data,
                                         iterations.ctypes.data)
        assert rc == 0
    assert np.isfinite(x).all() and np.isfinite(f).all() and (status != 1).all()     # no row ran into the iteration limit
    np.savez_compressed(OUT, x=x, f=f, status=status, num_iterations=iterations,
                        inputs_sha256=np.array(cases.inputs_digest(x0, lower, upper)))
    print("wrote %s: %d rows, iterations %d..%d" % (OUT, cases.B, iterations.min(), iterations.max()))


if __name__ == "__main__":
    main()
