"""The recorded Newton-descent cases (tests/golden/newton_descent_reference_vectors.npz, written by
tests/golden/make_golden_nd.py): a list of dicts with the inputs and the reference's results of every case.

`marked` (0 / 1 per case) is the generator's own finding on the CPU: the twin in device order (pairwise sums over the
padded width) against the twin in reference order (ascending sums) on the case's inputs misses the project's contract
— x* and f* within 1e-6 with equal status — on at least one row.  The two orders part in the last bits; a stalled search
or a loose stop then ends a solve at another iterate.  A marked case is compared with the reference on f* only, on the
rows where both converged; what the device must equal there byte for byte is its own twin.  The generator asserts the
caps below.

The cases named dense_... run the dense-Hessian functor (objective 101); the file keeps the integers they are built from
and digests of the larger results: see dense_cases.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newton_descent_reference_vectors.npz")
CONTRACT = 1e-6
MAX_MARKED_FRACTION = 0.25
NEVER_MARKED = ("scenario_verify_", "diag_quadratic_", "quartic_", "dense_spd_", "dense_single_", "dense_kappa0_",
                "dense_condition_")
CONVERGED = (3, 4)    # FDeltaViolation (the plateau test), GradientNormViolation


def misses_contract(a, b):
    """Rows on which two solves (x, f, g, progress) disagree beyond the contract.  (Equal infinities and rows that are
    NaN in both count as equal.)"""
    with np.errstate(invalid="ignore"):
        fx = np.abs(a[0] - b[0]) <= CONTRACT
        ff = np.abs(a[1] - b[1]) <= CONTRACT
    fx |= (a[0] == b[0]) | (np.isnan(a[0]) & np.isnan(b[0]))
    ff |= (a[1] == b[1]) | (np.isnan(a[1]) & np.isnan(b[1]))
    return ~(fx.all(axis=1) & ff & (a[3]["status"] == b[3]["status"]))


def load_cases():
    import dense_cases
    import nd_lib
    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files if "/" in k})
    cases = [dict(name=nm, **{k.split("/")[1]: z[k] for k in z.files if k.split("/")[0] == nm}) for nm in names]
    return cases + dense_cases.load(z, dict(stop=nd_lib.STOP_DTYPE, config=nd_lib.CONFIG_DTYPE,
                                            progress=nd_lib.PROGRESS_DTYPE))
