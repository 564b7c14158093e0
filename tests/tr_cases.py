"""The recorded trust-region cases (tests/golden/trust_region_reference_vectors.npz, written by
tests/golden/make_golden_tr.py): a list of dicts with the inputs and the reference's results of every case.

The cases named dense_... run the dense-Hessian functor (objective 101); the file keeps the integers they are built from
and digests of the larger results: see dense_cases.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trust_region_reference_vectors.npz")


def load_cases():
    import dense_cases
    import tr_lib
    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files if "/" in k})
    cases = [dict(name=nm, **{k.split("/")[1]: z[k] for k in z.files if k.split("/")[0] == nm}) for nm in names]
    return cases + dense_cases.load(z, dict(stop=tr_lib.STOP_DTYPE, config=tr_lib.CONFIG_DTYPE,
                                            progress=tr_lib.PROGRESS_DTYPE))
