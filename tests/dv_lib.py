"""ctypes helpers of the derivative-checker tests: the CPU twin (tests/derivatives/dv_twin.hpp, built by build() into
tests/derivatives/_build/), the device entry points, and — where the reference tree exists — the reference harness
compiled into a directory the caller names (tests/derivatives/ref_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DV_DIR = os.path.join(HERE, "derivatives")
REPO = os.path.dirname(HERE)
REFERENCE = "/root/reference"
TWIN_LIB = os.path.join(DV_DIR, "_build", "libdv_twin.so")
DV_LIBRARY = os.path.join(REPO, "cppnumericalsolvers_amd", "libmi355_lbfgs_dv.so")

ROSENBROCK, DIAG_QUADRATIC, QUARTIC, DENSE, PLANTED, L1_QUADRATIC = 0, 1, 100, 101, 102, 103
REF_ORDER, DEVICE_ORDER = 0, 1
CONFIG_FIELDS = ("gradient_accuracy", "hessian_accuracy", "gradient_step", "hessian_step", "gradient_tolerance",
                 "hessian_tolerance")
CONFIG_DTYPE = np.dtype([("gradient_accuracy", "<i4"), ("hessian_accuracy", "<i4"), ("gradient_step", "<f8"),
                         ("hessian_step", "<f8"), ("gradient_tolerance", "<f8"), ("hessian_tolerance", "<f8")], align=True)
REPORT_DTYPE = np.dtype([("gradient_ok", "<i4"), ("hessian_ok", "<i4"), ("gradient_worst_index", "<i4"),
                         ("hessian_worst_index", "<i4"), ("nonfinite", "<i4"), ("pad", "<i4"),
                         ("gradient_worst_excess", "<f8"), ("hessian_worst_excess", "<f8")], align=True)
assert CONFIG_DTYPE.itemsize == 40 and REPORT_DTYPE.itemsize == 40
OUTPUTS = ("f", "grad", "grad_fd", "hess", "hess_fd", "report")


def make_config(cfg):
    c = np.zeros(1, dtype=CONFIG_DTYPE)
    for k in CONFIG_FIELDS:
        c[k] = cfg[k]
    return c


def library_mapping(n):
    """(W, E) the library picks for lanes_per_problem = 0."""
    W = 8
    while W < n and W < 64:
        W *= 2
    return W, (1 if n <= W else (2 if n <= 2 * W else 4))


def _outputs(B, n, hessian):
    out = dict(f=np.zeros(B), grad=np.zeros((B, n)), grad_fd=np.zeros((B, n)),
               hess=np.zeros((B, n, n)) if hessian else None, hess_fd=np.zeros((B, n, n)) if hessian else None,
               report=np.zeros(B, dtype=REPORT_DTYPE))
    return out


def _pointer(a):
    return a.ctypes.data if a is not None else None


_twin = None


def twin_check(objective, x, params=None, cfg=None, order=DEVICE_ORDER, hessian=True, lanes=0):
    """The CPU twin on every row of x: dict of f, grad, grad_fd, hess, hess_fd ([B, n, n], entry [b, j, i] = H(i, j)),
    report.  lanes: an explicit lanes_per_problem of the device order (0: the library's mapping)."""
    global _twin
    if _twin is None:
        _twin = C.CDLL(TWIN_LIB)
        _twin.dv_twin_check.restype = C.c_int
        _twin.dv_twin_check.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + \
                                       [C.c_void_p] * 7
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, n = x.shape
    W, E = library_mapping(n)
    if lanes:
        W, E = lanes, (1 if n <= lanes else (2 if n <= 2 * lanes else 4))
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    out = _outputs(B, n, hessian)
    c = make_config(cfg)
    rc = _twin.dv_twin_check(objective, n, B, params.ctypes.data, c.ctypes.data, order, W * E, E, x.ctypes.data,
                             *[_pointer(out[k]) for k in OUTPUTS])
    assert rc == 0, "unsupported twin check"
    return out


def device_objective(amd, objective, params, n):
    if objective == ROSENBROCK:
        return amd.Rosenbrock()
    if objective == DIAG_QUADRATIC:
        return amd.DiagQuadratic(params[:n], float(params[n]))
    return amd.Objective(int(objective), np.ascontiguousarray(params, dtype=np.float64) if objective in (DENSE, PLANTED, L1_QUADRATIC)
                         else np.zeros(0), "user")


def desc_for(amd, objective, params, n, lanes=0, arithmetic=0):
    from cppnumericalsolvers_amd import capi
    obj = device_objective(amd, objective, params, n)
    d = capi.Desc()
    d.objective = obj.objective_id
    d.n = int(n)
    d.m = 1
    p = np.ascontiguousarray(obj.params, dtype=np.float64)
    d.objective_params = p.ctypes.data_as(C.POINTER(C.c_double)) if p.size else None
    d.n_params = int(p.size)
    d.lanes_per_problem = int(lanes)
    d.arithmetic = int(arithmetic)
    return d, p


def device_check(ctx, objective, x, params=None, cfg=None, hessian=True, lanes=0, host=False, skip=(), arithmetic=0,
                 check=True):
    """mi355_check_derivatives_batch (or _host) on ctx's library: the same dict as twin_check.  skip: outputs passed as
    NULL (their entries come back None).  check=False: returns (rc, message) instead of raising."""
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, n = x.shape
    d, keep = desc_for(amd, objective, params, n, lanes, arithmetic)
    c = capi.DerivativeConfig(*[cfg[k] for k in CONFIG_FIELDS]) if cfg is not None else None
    out = _outputs(B, n, hessian)
    for k in skip:
        out[k] = None
    cp = C.byref(c) if c is not None else None
    if host:
        rc = ctx._lib.mi355_check_derivatives_batch_host(ctx.handle, C.byref(d), cp, B, x.ctypes.data,
                                                         *[_pointer(out[k]) for k in OUTPUTS])
    else:
        dev = {k: (torch.from_numpy(v.view(np.uint8).reshape(-1).copy()).to("cuda:0") if v is not None else None)
               for k, v in out.items()}
        xd = torch.from_numpy(x).to("cuda:0")
        rc = ctx._lib.mi355_check_derivatives_batch(ctx.handle, C.byref(d), cp, B, xd.data_ptr(),
                                                    *[(dev[k].data_ptr() if dev[k] is not None else None) for k in OUTPUTS],
                                                    None)
        torch.cuda.synchronize()
        for k, v in out.items():
            if v is not None:
                out[k] = dev[k].cpu().numpy().view(v.dtype).reshape(v.shape)
    del keep
    if not check:
        return rc, (ctx._lib.mi355_lbfgs_last_error() or b"").decode()
    capi.check(rc)
    return out


def same_bits(a, b, what=""):
    """None, or a description of the first difference between two result dicts (NaNs compare by their bytes)."""
    for k in OUTPUTS:
        if a.get(k) is None or b.get(k) is None:
            continue
        ab, bb = np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)
        if ab.shape != bb.shape or not (ab == bb).all():
            if k == "report":
                return "%s report: %r != %r" % (what, a[k], b[k])
            bad = np.argwhere(np.ascontiguousarray(a[k]).view(np.uint64) != np.ascontiguousarray(b[k]).view(np.uint64))
            i = tuple(bad[0])
            return "%s %s%s: %r != %r (%d entries differ)" % (what, k, i, a[k][i], b[k][i], len(bad))
    return None


def build_reference(out_dir):
    """Compile the reference harness over the reference tree into out_dir; returns the library path."""
    lib = os.path.join(out_dir, "libdv_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                           "-I" + os.path.join(REPO, "oracle", "eigen_shim"),
                           "-I" + os.path.join(REFERENCE, "include"), "-I" + DV_DIR,
                           os.path.join(DV_DIR, "ref_harness.cpp"), "-o", lib])
    return lib


def reference_check(lib_path, objective, x, params=None, cfg=None):
    """The reference's ComputeFiniteGradient / ComputeFiniteHessian / IsGradientCorrect / IsHessianCorrect on every row of
    x: dict of grad_fd, hess_fd ([B, n, n], entry [b, j, i] = H(i, j)), gradient_ok, hessian_ok."""
    L = C.CDLL(lib_path)
    L.dv_ref_check.restype = C.c_int
    L.dv_ref_check.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    x = np.ascontiguousarray(x, dtype=np.float64)
    B, n = x.shape
    params = np.ascontiguousarray(params if params is not None else np.zeros(1), dtype=np.float64)
    out = dict(grad_fd=np.zeros((B, n)), hess_fd=np.zeros((B, n, n)), gradient_ok=np.zeros(B, dtype=np.int32),
               hessian_ok=np.zeros(B, dtype=np.int32))
    rc = L.dv_ref_check(objective, n, B, params.ctypes.data, int(cfg["gradient_accuracy"]), int(cfg["hessian_accuracy"]),
                        x.ctypes.data, out["grad_fd"].ctypes.data, out["hess_fd"].ctypes.data,
                        out["gradient_ok"].ctypes.data, out["hessian_ok"].ctypes.data)
    assert rc == 0, "unsupported reference check"
    return out
