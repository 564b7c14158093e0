"""Writes tests/golden/lbfgs_f32_reference.npz: the reference's Lbfgs<F, m, MoreThuente> on float functors
(tests/lbfgs_f32/ref_harness.cpp over the reference tree and oracle/eigen_shim, compiled into a temporary directory
outside the repository) on the cases of tests/l32_cases.py.  Needs the reference tree; run from the repository root:
    python tests/golden/make_golden_f32.py
The file holds results only (the inputs are rebuilt from the case names and the recorded seed)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import l32_cases as Cs  # noqa: E402
import l32_lib as L  # noqa: E402


def reference_record(ref, case):
    x, f, g, prog = ref(case["objective"], case["m"], case["x0"], case["params"], case["stop"])
    _, _, _, _, rows, xs = ref.trajectory(case["objective"], case["m"], case["x0"][0], case["params"], case["stop"])
    return Cs.record_of(case, x, f, g, prog, rows, xs)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ref = L.reference_solver(L.build_reference(tmp))
        records = {case["name"]: reference_record(ref, case) for case in Cs.all_cases()}
    np.savez_compressed(Cs.GOLDEN, **Cs.pack(Cs.all_cases(), records))
    print("%s: %d cases, %d bytes" % (Cs.GOLDEN, len(Cs.all_cases()), os.path.getsize(Cs.GOLDEN)))


if __name__ == "__main__":
    main()
