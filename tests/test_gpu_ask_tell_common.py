"""The contract the three ask/tell handles share, run on each through the C entry points: mi355_lbfgs_ask_tell_*
(double), mi355_lbfgs_ask_tell_f32_* (float) and mi355_lbfgsb_ask_tell_* (Lbfgsb, double).

1. B = 3, n = 5, m = 3: no part of the state is a multiple of 16 bytes long (the float evaluation buffer is 60 bytes), yet
   _x is 16-byte aligned and _active 8-byte aligned; _results before the first step returns the bits of x0, status
   NOT_STARTED and nfev 0; one _step fed the library's own evaluation of _x leaves all three active; _destroy is OK.
2. B = 0: create, step with null f and g, results and destroy are OK, and step reports 0 active.
3. A desc that trips two refusals reports the one that stands first in the path's sequence (the messages were recorded
   before the three entry units were merged into one)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NOT_STARTED = -1

PATHS = {
    "lbfgs": dict(prefix="mi355_lbfgs_ask_tell_", dtype=np.float64, box=False),
    "lbfgs_f32": dict(prefix="mi355_lbfgs_ask_tell_f32_", dtype=np.float32, box=False),
    "lbfgsb": dict(prefix="mi355_lbfgsb_ask_tell_", dtype=np.float64, box=True),
}


def _amd():
    import cppnumericalsolvers_amd as amd
    return amd


@pytest.fixture(scope="module")
def context():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    ctx = _amd().Context(0)
    yield ctx
    ctx.close()


class _View:
    """device memory the library owns, for torch.as_tensor (no copy)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(int(ptr), False), version=2, strides=None)


def _desc(n, m, **over):
    from cppnumericalsolvers_amd import capi
    d = capi.Desc()
    d.objective, d.linesearch, d.n, d.m = capi.OBJ_ROSENBROCK, capi.LS_MORE_THUENTE, n, m
    d.stop = capi.default_stop()
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _create(lib, path, ctx, d, B, x0_ptr, h):
    fn = getattr(lib, path["prefix"] + "create")
    if path["box"]:
        return fn(ctx.handle, C.byref(d), None, None, 0, B, x0_ptr, None, C.byref(h))
    return fn(ctx.handle, C.byref(d), B, x0_ptr, None, C.byref(h))


@pytest.mark.parametrize("name", sorted(PATHS))
def test_odd_sizes_alignment_first_results_and_one_step(context, name):
    import torch
    amd = _amd()
    from cppnumericalsolvers_amd import capi
    path, lib = PATHS[name], context._lib
    call = lambda what, *a: capi.check(getattr(lib, path["prefix"] + what)(*a))  # noqa: E731
    B, n, m = 3, 5, 3
    dtype = path["dtype"]
    tdtype = torch.float32 if dtype == np.float32 else torch.float64
    x0 = np.array([[-1.2 + 0.3 * b + 0.07 * j * (-1) ** j for j in range(n)] for b in range(B)], dtype=dtype)
    x0d = torch.from_numpy(x0).to("cuda:0")
    h = C.c_void_p()
    capi.check(_create(lib, path, context, _desc(n, m), B, x0d.data_ptr(), h))
    try:
        xp, ap = C.c_void_p(), C.c_void_p()
        call("x", h, C.byref(xp))
        call("active", h, C.byref(ap))
        assert xp.value % 16 == 0, hex(xp.value)
        assert ap.value % 8 == 0, hex(ap.value)
        x = torch.empty(B, n, dtype=tdtype, device="cuda:0")
        g = torch.empty(B, n, dtype=tdtype, device="cuda:0")
        f = torch.empty(B, dtype=tdtype, device="cuda:0")
        prog = torch.empty(B * capi.PROGRESS_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        call("results", h, x.data_ptr(), f.data_ptr(), g.data_ptr(), prog.data_ptr(), None)
        torch.cuda.synchronize()
        assert x.cpu().numpy().tobytes() == x0.tobytes()
        p = amd.progress_to_numpy(prog)
        assert np.all(p["status"] == NOT_STARTED) and np.all(p["nfev"] == 0), p
        # the library's own evaluation of the points asked for
        solver = amd.BatchedLbfgs(m=m, context=context, arithmetic="exact", dtype=tdtype)
        asked = torch.as_tensor(_View(xp.value, (B, n), "<f4" if dtype == np.float32 else "<f8"), device="cuda:0")
        assert asked.cpu().numpy().tobytes() == x0.tobytes()
        fe, ge = solver.evaluate(amd.Rosenbrock(), asked)
        count = C.c_int64(-1)
        call("step", h, fe.data_ptr(), ge.data_ptr(), C.byref(count), None)
        assert count.value == 3
        assert int(torch.as_tensor(_View(ap.value, (1,), "<i8"), device="cuda:0").item()) == 3
    finally:
        rc = getattr(lib, path["prefix"] + "destroy")(h)
    assert rc == capi.MI355_OK


@pytest.mark.parametrize("name", sorted(PATHS))
def test_empty_batch(context, name):
    from cppnumericalsolvers_amd import capi
    path, lib = PATHS[name], context._lib
    h = C.c_void_p()
    assert _create(lib, path, context, _desc(5, 3), 0, None, h) == capi.MI355_OK and h.value
    count = C.c_int64(-1)
    assert getattr(lib, path["prefix"] + "step")(h, None, None, C.byref(count), None) == capi.MI355_OK
    assert count.value == 0
    assert getattr(lib, path["prefix"] + "results")(h, None, None, None, None, None) == capi.MI355_OK
    assert getattr(lib, path["prefix"] + "destroy")(h) == capi.MI355_OK


# the message of a desc that trips two refusals at once, as the separate entry units reported it
FIRST_OF_TWO = {
    "lbfgs": "Lbfgs ask/tell is built with the More-Thuente line search only (no Hager-Zhang)",
    "lbfgs_f32": "Lbfgs ask/tell f32 is built with the More-Thuente line search only (no Hager-Zhang)",
    "lbfgsb": "Lbfgsb ask/tell is built for the reference-order arithmetic only (no MI355_ARITH_FMA",
}


@pytest.mark.parametrize("name", sorted(PATHS))
def test_the_first_of_two_refusals_is_reported(context, name):
    import torch
    amd = _amd()
    from cppnumericalsolvers_amd import capi
    path, lib = PATHS[name], context._lib
    if path["box"]:
        d = _desc(8, 9, arithmetic=capi.ARITH_FMA)                      # ... and m = 9 > 8
    else:
        trace = amd.Trace([0], 4, 8, "cuda:0")
        d = _desc(8, 6, linesearch=capi.LS_HAGER_ZHANG, trace=trace.c_pointer())
    x0 = torch.zeros(4, 8, dtype=torch.float32 if path["dtype"] == np.float32 else torch.float64, device="cuda:0")
    h = C.c_void_p()
    rc = _create(lib, path, context, d, 4, x0.data_ptr(), h)
    message = lib.mi355_lbfgs_last_error().decode()
    assert rc == capi.ERR_UNSUPPORTED and not h.value, (rc, message)
    assert FIRST_OF_TWO[name] in message, message
    assert "trace" not in message and "m <= 8" not in message, message
