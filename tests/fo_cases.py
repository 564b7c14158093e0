"""The recorded first-order cases (tests/golden/first_order_reference_vectors.npz, written by
tests/golden/make_golden_fo.py): a list of dicts with the inputs and the reference's results of every case, for
GradientDescent (names gd_...) and ConjugatedGradientDescent (cg_...).

`marked` (0 / 1 per case) is the generator's own finding on the CPU: the twin in device order (pairwise sums over the
padded width) against the twin in reference order (ascending sums) on the case's inputs misses the project's contract
— x* and f* within 1e-6 with equal status — on at least one row.  The two orders part in the last bits, and a
first-order iteration on Rosenbrock amplifies that until a capped solve ends at another iterate.  A marked case is
compared with the reference on f* only, on the rows where both converged; what the device must equal there byte for
byte is its own twin.  The generator asserts the caps below.

Size.  The file may not outgrow the Newton-descent one, and x and g of eleven dimensions up to 256, eight rows, two stops
and two solvers are 0.8 MB of incompressible doubles.  Two measures keep every case the issue names: the Rosenbrock
starts are 1 + s k / 128 with integer k (stored as int16 `x0_q` and the per-row s `x0_scale`; `x0` is rebuilt here,
exactly), and above n = 33 the reference's x and g are recorded as SHA-256 digests of their bytes (`x_sha256`,
`g_sha256`) beside f and the progress fields in full.  A digest serves the bit-for-bit comparison as the bytes do; where a
test needs the reference's x as numbers it takes the twin in reference order after checking its digest against the
recorded one (reference_x)."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_order_reference_vectors.npz")
CONTRACT = 1e-6
MAX_MARKED_FRACTION = 0.25
NEVER_MARKED = ("scenario_verify_", "diag_quadratic_")
CONVERGED = (3, 4)    # FDeltaViolation (the plateau test), GradientNormViolation
FULL_RECORD_MAX_N = 33


def starts_from(k, scale):
    """x0 = 1 + s k / 128 (the chained Rosenbrock's minimiser is 1), row by row"""
    return 1.0 + scale[:, None] * (k.astype(np.float64) / 128.0)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


def same_as_recorded(case, key, a):
    """a (the twin's x or g in reference order) against the reference's recorded bytes, or their digest"""
    if key in case:
        return a.tobytes() == case[key].tobytes()
    return digest(a).tobytes() == case[key + "_sha256"].tobytes()


def reference_x(case, twin_x):
    """The reference's x*: recorded, or — digest cases — the reference-order twin's, which must have the recorded digest"""
    if "x" in case:
        return case["x"]
    assert same_as_recorded(case, "x", twin_x), case["name"] + ": the twin in reference order is not the recorded x"
    return twin_x


def never_marked(name):
    return name.split("_", 1)[1].startswith(NEVER_MARKED)


def misses_contract(a, b):
    """Rows on which two solves (x, f, g, progress) disagree beyond the contract.  (Equal infinities and rows that are
    NaN in both count as equal.)"""
    with np.errstate(invalid="ignore"):
        fx = np.abs(a[0] - b[0]) <= CONTRACT
        ff = np.abs(a[1] - b[1]) <= CONTRACT
    fx |= (a[0] == b[0]) | (np.isnan(a[0]) & np.isnan(b[0]))
    ff |= (a[1] == b[1]) | (np.isnan(a[1]) & np.isnan(b[1]))
    return ~(fx.all(axis=1) & ff & (a[3]["status"] == b[3]["status"]))


def pack(arrays):
    """{"case/key": array} -> the few arrays of the file: one blob per dtype and a JSON index (a zip member per array
    would cost more bytes than most of these arrays hold)"""
    blobs, index = {}, {}
    for name, a in arrays.items():
        a = np.require(np.asarray(a), requirements="C")
        kind = a.dtype.str if a.dtype.names is None else "V:" + name.split("/")[1]
        raw = a.reshape(-1).view(np.uint8) if a.dtype.names is not None else a.reshape(-1)
        chunks = blobs.setdefault(kind, [])
        offset = sum(len(c) for c in chunks)
        chunks.append(raw)
        index[name] = [kind, list(a.shape), offset, len(raw)]
    out = {"blob_%d" % i: np.concatenate(v) for i, (k, v) in enumerate(sorted(blobs.items()))}
    kinds = [k for k, _ in sorted(blobs.items())]
    out["index"] = np.frombuffer(json.dumps(dict(kinds=kinds, arrays=index)).encode(), dtype=np.uint8)
    return out


def unpack(z, struct_dtypes):
    meta = json.loads(z["index"].tobytes().decode())
    blobs = {k: z["blob_%d" % i] for i, k in enumerate(meta["kinds"])}
    out = {}
    for name, (kind, shape, offset, length) in meta["arrays"].items():
        raw = blobs[kind][offset:offset + length]
        if kind.startswith("V:"):
            out[name] = raw.copy().view(struct_dtypes[kind[2:]]).reshape(shape)
        else:
            out[name] = raw.reshape(shape).copy()
    return out


def load_cases():
    import fo_lib
    arrays = unpack(np.load(GOLDEN), dict(stop=fo_lib.STOP_DTYPE, config=fo_lib.CONFIG_DTYPE,
                                          progress=fo_lib.PROGRESS_DTYPE))
    names = sorted({k.split("/")[0] for k in arrays})
    cases = [dict(name=nm, **{k.split("/")[1]: v for k, v in arrays.items() if k.split("/")[0] == nm}) for nm in names]
    for c in cases:
        if "x0" not in c:
            c["x0"] = starts_from(c["x0_q"], c["x0_scale"])
    return cases
