"""The recorded Nelder-Mead cases (tests/golden/nelder_mead_reference_vectors.npz, written by
tests/golden/make_golden_nm.py): a list of dicts with the inputs and the reference's results of every case."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nelder_mead_reference_vectors.npz")
MAX_TIED_FRACTION = 0.05   # of the problems of a case; make_golden_nm.py asserts it when it writes the file


def load_cases():
    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files})
    return [dict(name=nm, **{k.split("/")[1]: z[k] for k in z.files if k.split("/")[0] == nm}) for nm in names]


def comparable(tied, *values):
    """The solves whose comparison with the reference is claimed: no tie in any ranking, finite values throughout; at
    most MAX_TIED_FRACTION of a case may drop out through ties."""
    tied = np.asarray(tied, dtype=bool)
    assert tied.mean() <= MAX_TIED_FRACTION, "more than 5 % of the case's solves met a tie"
    ok = ~tied
    for v in values:
        v = np.asarray(v, dtype=np.float64)
        ok &= np.isfinite(v.reshape(len(tied), -1)).all(axis=1)
    return ok
