"""Records what the reference's UNMODIFIED utils/derivatives.h returns on the cases of tests/dv_cases.py:
tests/golden/derivatives_reference_vectors.npz.  Needs the reference tree; the harness (tests/derivatives/ref_harness.cpp)
is compiled into a temporary directory and nothing built from it is kept.

Per case `<name>`: x, params, the accuracies, grad_fd, gradient_ok, hessian_ok and hess_fd — the n x n blocks in full up to
n = 33, as one SHA-256 digest of the [B, n, n] array above (dv_cases.DIGEST_ABOVE).  Cases with a step override are not
recorded (the reference has none); the Hessian of a gradient-only case is recorded up to n = 64 all the same.

The margin rule of the pass and planted cases is a condition on these INPUTS and is asserted here, on the CPU twin in both
summation orders: worst excess < 0.5 where a verdict must pass, > 2 where it must fail.  A case that lands in between is
replaced in dv_cases.py, not tolerated.

    python tests/golden/make_golden_dv.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dv_cases  # noqa: E402
import dv_lib as T  # noqa: E402


def assert_margins(case):
    for order in (T.REF_ORDER, T.DEVICE_ORDER):
        rep = T.twin_check(case["objective"], case["x"], case["params"], case["config"], order=order,
                           hessian=case["hessian"])["report"]
        checked = ("gradient", "hessian") if case["hessian"] else ("gradient",)
        for which in checked:
            excess = rep[which + "_worst_excess"]
            must_fail = case["kind"] == "planted" and (case["fails"] == which or case.get("other_fails"))
            assert (excess > 2.0).all() if must_fail else (excess < 0.5).all(), (case["name"], order, which, excess)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = T.build_reference(tmp)
        for case in dv_cases.make_cases():
            if case["kind"] in ("pass", "planted"):
                assert_margins(case)
            n = case["x"].shape[1]
            if n > 64 or case["config"]["hessian_step"] or case["config"]["gradient_step"]:
                continue
            r = T.reference_check(lib, case["objective"], case["x"], case["params"], case["config"])
            name = case["name"]
            out[name + "/x"] = case["x"]
            out[name + "/params"] = case["params"]
            out[name + "/accuracy"] = np.array([case["config"]["gradient_accuracy"], case["config"]["hessian_accuracy"]],
                                               dtype=np.int32)
            out[name + "/grad_fd"] = r["grad_fd"]
            out[name + "/gradient_ok"] = r["gradient_ok"]
            out[name + "/hessian_ok"] = r["hessian_ok"]
            if n <= dv_cases.DIGEST_ABOVE:
                out[name + "/hess_fd"] = r["hess_fd"]
            else:
                out[name + "/hess_fd_sha256"] = np.array(dv_cases.digest(r["hess_fd"]))
    np.savez_compressed(dv_cases.GOLDEN, **out)
    print("%s: %d arrays, %d bytes" % (dv_cases.GOLDEN, len(out), os.path.getsize(dv_cases.GOLDEN)))


if __name__ == "__main__":
    main()
