"""The recorded trust-region cases (tests/golden/trust_region_reference_vectors.npz, written by
tests/golden/make_golden_tr.py): a list of dicts with the inputs and the reference's results of every case."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trust_region_reference_vectors.npz")


def load_cases():
    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files})
    return [dict(name=nm, **{k.split("/")[1]: z[k] for k in z.files if k.split("/")[0] == nm}) for nm in names]
