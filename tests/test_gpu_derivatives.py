"""The derivative checker on the MI355X (csrc/derivative_check_kernel.hpp): bit for bit the CPU twin in device order on every
case and under wider lane mappings, the functor's gradient equal to mi355_lbfgs_eval_batch's, the dense quartic's Hessian
equal to the one tests/dense_cases.py builds, host entry point == device entry point == Python API, NULL outputs, the
verdicts of the pass and planted cases, the wider Hessian step on the noise-dominated start, clean refusals, and the C++
header test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dv_cases
import dv_lib as T

pytestmark = pytest.mark.gpu
CASES = dv_cases.make_cases()
BY_NAME = {c["name"]: c for c in CASES}
_contexts = {}


def _context(objective):
    """One context on the default library, one on the library that holds the user functors' derivative kernels."""
    import cppnumericalsolvers_amd as amd
    key = "dv" if objective >= 100 else "default"
    if key not in _contexts:
        _contexts[key] = amd.Context(0, library=T.DV_LIBRARY if key == "dv" else None)
    return _contexts[key]


def _device(case, **kw):
    return T.device_check(_context(case["objective"]), case["objective"], case["x"], case["params"], case["config"],
                          hessian=case["hessian"], **kw)


def _twin(case, **kw):
    return T.twin_check(case["objective"], case["x"], case["params"], case["config"], order=T.DEVICE_ORDER,
                        hessian=case["hessian"], **kw)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_matches_twin(case):
    out = _device(case)
    diff = T.same_bits(out, _twin(case), case["name"])
    assert diff is None, diff
    rep = out["report"]
    if case["kind"] == "pass":
        assert (rep["gradient_ok"] == 1).all() and (rep["hessian_ok"] == 1).all(), rep
    if case["kind"] == "planted":
        which = case["fails"]
        assert (rep[which + "_ok"] == 0).all(), rep
        if case["worst_index"] is not None:
            assert (rep[which + "_worst_index"] == case["worst_index"]).all(), rep
        else:
            assert np.isin(rep[which + "_worst_index"], case["worst_among"]).all(), rep
        other = "hessian" if which == "gradient" else "gradient"
        if case["hessian"] and not case.get("other_fails"):
            assert (rep[other + "_ok"] == 1).all(), rep


@pytest.mark.parametrize("name,lanes", [
    ("grad_rosenbrock_n009_a3", (16, 64)), ("grad_diag_quadratic_n017_a2", (32, 64)), ("grad_planted_n009_a3", (16, 32, 64)),
    ("grad_dense_n017_a3", (64,)), ("grad_quartic_n009_a0", (64,)), ("hess_rosenbrock_n09_a3", (16, 32, 64)),
    ("hess_rosenbrock_n16_a0", (32, 64)), ("hess_diag_quadratic_n09_a3", (64,)), ("hess_dense_n08_a3", (16, 64)),
    ("planted_hessian_n17_i07_j08", (64,)), ("special_rosenbrock_n09", (32,))])
def test_wider_lanes_same_bits(name, lanes):
    """Zero padding adds zeros to every tree: an explicit wider lanes_per_problem gives the bytes of the padded width."""
    case = BY_NAME[name]
    first = _device(case)
    for w in lanes:
        diff = T.same_bits(first, _device(case, lanes=w), "%s at %d lanes" % (name, w))
        assert diff is None, diff


@pytest.mark.parametrize("name", ["grad_rosenbrock_n033_a2", "grad_rosenbrock_n129_a1", "grad_diag_quadratic_n065_a1",
                                  "grad_diag_quadratic_n256_a3"])
def test_gradient_equals_eval_batch(name):
    import torch
    import cppnumericalsolvers_amd as amd
    case = BY_NAME[name]
    n = case["x"].shape[1]
    W, E = T.library_mapping(n)
    solver = amd.BatchedLbfgs(context=_context(0), arithmetic="exact", lanes_per_problem=W, elems_per_lane=E)
    f, g = solver.evaluate(T.device_objective(amd, case["objective"], case["params"], n),
                           torch.from_numpy(case["x"]).to("cuda:0"))
    torch.cuda.synchronize()
    out = _device(case)
    assert (g.cpu().numpy().view(np.uint64) == out["grad"].view(np.uint64)).all()
    assert (f.cpu().numpy().view(np.uint64) == out["f"].view(np.uint64)).all()


def test_dense_hessian_equals_dense_cases_twin():
    """hess of the dense quartic on the cases of tests/dense_cases.py (S never symmetrised, one with S != S^T): the H its
    twin builds."""
    import dense_cases
    for n, flags in ((9, 0), (17, dense_cases.ASYMMETRIC), (33, 0)):
        ints = dense_cases.integers(20261019, n, flags=flags, rows=5)
        p, x = dense_cases.params(ints), dense_cases.starts(ints)
        out = T.device_check(_context(T.DENSE), T.DENSE, x, p, dv_cases.config(0), hessian=True)
        for b in range(x.shape[0]):
            H = dense_cases.hessian(p, x[b])   # [i, j]; the device array is column major: [b, j, i]
            assert (np.ascontiguousarray(out["hess"][b].T).view(np.uint64) == H.view(np.uint64)).all(), (n, b)


@pytest.mark.parametrize("name", ["grad_rosenbrock_n017_a1", "hess_rosenbrock_n17_a3", "hess_dense_n09_a0",
                                  "planted_one_sided_n17_i08_j07"])
def test_host_entry_point_equals_device(name):
    case = BY_NAME[name]
    diff = T.same_bits(_device(case, host=True), _device(case), name)
    assert diff is None, diff


@pytest.mark.parametrize("skip", [("f",), ("grad",), ("grad_fd",), ("hess",), ("hess_fd",), ("report",),
                                  ("f", "grad", "grad_fd", "hess", "hess_fd"), ("grad", "grad_fd", "hess", "hess_fd", "report"),
                                  ("hess", "hess_fd")])
def test_null_outputs(skip):
    """Every output may be NULL: the others keep their bytes, the report too (its missing sides go to temporaries)."""
    case = BY_NAME["hess_rosenbrock_n09_a3"]
    full = _device(case)
    if skip == ("hess", "hess_fd"):   # both Hessian outputs NULL: gradient only, the Hessian is not checked
        part = _device(case, skip=skip)
        assert (part["report"]["hessian_ok"] == -1).all()
        for k in ("f", "grad", "grad_fd"):
            assert (part[k].view(np.uint64) == full[k].view(np.uint64)).all()
        return
    part = _device(case, skip=skip)
    if "hess" in skip and "hess_fd" in skip and "report" not in skip:   # (with the report alone too: no Hessian output, no Hessian check)
        assert (part["report"]["hessian_ok"] == -1).all() and (part["report"]["hessian_worst_index"] == -1).all()
        for k in ("gradient_ok", "gradient_worst_index", "gradient_worst_excess"):
            assert (part["report"][k] == full["report"][k]).all(), k
        part["report"] = None
    diff = T.same_bits(part, full, "skip %r" % (skip,))
    assert diff is None, diff


@pytest.mark.parametrize("name", ["hess_rosenbrock_n09_a3", "pass_rosenbrock_wide_step_n09", "grad_diag_quadratic_n065_a1"])
def test_python_api_same_bytes(name):
    import torch
    import cppnumericalsolvers_amd as amd
    case = BY_NAME[name]
    n = case["x"].shape[1]
    c = case["config"]
    r = amd.check_derivatives(T.device_objective(amd, case["objective"], case["params"], n),
                              torch.from_numpy(case["x"]).to("cuda:0"), hessian=case["hessian"],
                              accuracy=c["gradient_accuracy"], gradient_step=c["gradient_step"],
                              hessian_step=c["hessian_step"], gradient_tolerance=c["gradient_tolerance"],
                              hessian_tolerance=c["hessian_tolerance"], context=_context(case["objective"]))
    torch.cuda.synchronize()
    got = dict(f=r.f.cpu().numpy(), grad=r.grad.cpu().numpy(), grad_fd=r.grad_fd.cpu().numpy(),
               hess=r.hess.cpu().numpy() if case["hessian"] else None,
               hess_fd=r.hess_fd.cpu().numpy() if case["hessian"] else None,
               report=r.report.cpu().numpy().view(T.REPORT_DTYPE))
    want = _device(case)
    diff = T.same_bits(got, want, name)
    assert diff is None, diff
    for k in ("gradient_ok", "hessian_ok", "gradient_worst_index", "hessian_worst_index", "nonfinite",
              "gradient_worst_excess", "hessian_worst_excess"):
        assert (getattr(r, k).cpu().numpy() == want["report"][k]).all(), k


def test_wider_hessian_step_turns_noise_into_pass():
    """Rosenbrock at an ordinary start: the reference's step fails a correct Hessian (rounding noise of the size of f in
    the second difference), hessian_step = 2^-13 passes it."""
    case = BY_NAME["hess_rosenbrock_n09_a3"]
    assert (_device(case)["report"]["hessian_ok"] == 0).all()
    wide = dict(case, config=dict(case["config"], hessian_step=dv_cases.WIDE_STEP))
    rep = _device(wide)["report"]
    assert (rep["hessian_ok"] == 1).all() and (rep["hessian_worst_excess"] < 0.5).all(), rep


def test_nonfinite_entries_pass_and_are_counted():
    case = BY_NAME["special_rosenbrock_n09"]
    rep = _device(case)["report"]
    n = case["x"].shape[1]
    # the row with 1e200: f overflows, every finite-difference entry is NaN, and every one of them passes
    assert rep["nonfinite"][2] == n + n * n and rep["gradient_ok"][2] == 1 and rep["hessian_ok"][2] == 1
    assert (rep["nonfinite"][[0, 3, 4]] == 0).all()


def test_value_only_functor_finite_gradient():
    """examples/user_objective_l1 has a value and nothing else: the finite gradient alone."""
    n = 9
    c = np.linspace(-1.0, 1.0, n)
    x = dv_cases.mixed_points(5, n, 9)
    out = T.device_check(_context(T.L1_QUADRATIC), T.L1_QUADRATIC, x, c, dv_cases.config(3), hessian=False,
                         skip=("grad",))
    # d/dx (|d| + 0.5 d^2) = sign(d) + d away from the kink; the 8-point stencil of a piecewise quadratic whose kink is
    # farther than 4 h ~ 6e-8 max(|x|, 1) away is exact up to rounding of f (|f| <= 50, eps |f| / h ~ 1e-6)
    d = x - c
    assert np.abs(d).min() > 1e-6
    np.testing.assert_allclose(out["grad_fd"], np.sign(d) + d, rtol=0, atol=1e-5)
    assert (out["report"]["gradient_ok"] == -1).all()


REFUSALS = [
    ("gradient_n257", dict(objective=T.ROSENBROCK, n=257, hessian=False), -4, "n <= 256"),
    ("hessian_n65", dict(objective=T.ROSENBROCK, n=65, hessian=True), -4, "n <= 64"),
    ("fma", dict(objective=T.ROSENBROCK, n=9, hessian=False, arithmetic=2), -4, "MI355_ARITH_FMA"),
    ("hessian_without_hess_full", dict(objective=T.L1_QUADRATIC, n=9, hessian=True, skip=("grad", "grad_fd", "f", "report")),
     -4, "no hess_full"),
    ("gradient_of_value_only", dict(objective=T.L1_QUADRATIC, n=9, hessian=False), -4, "no eval"),
]


@pytest.mark.parametrize("name,kw,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, kw, code, text):
    kw = dict(kw)
    n = kw.pop("n")
    objective = kw.pop("objective")
    x = np.zeros((2, n))
    params = np.zeros(n) if objective == T.L1_QUADRATIC else None
    rc, msg = T.device_check(_context(objective), objective, x, params, dv_cases.config(3), check=False, **kw)
    assert rc == code and text in msg, (rc, msg)


def test_refuses_ridge_and_library_without_derivative_kernels():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    x = torch.zeros(2, 8, dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.EngineError) as e:
        # (the ridge objective's own validation wants its per-problem rows: the refusal must name the LDS data instead)
        obj = amd.SquaredErrorRidge(np.ones((4, 8)), 0.5)
        d, keep = T.desc_for(amd, 0, None, 8)
        d.objective = obj.objective_id
        p = np.ascontiguousarray(obj.params)
        d.objective_params = p.ctypes.data_as(C.POINTER(C.c_double))
        d.n_params = int(p.size)
        y = torch.zeros(2, 4, dtype=torch.float64, device="cuda:0")
        d.per_problem_data = y.data_ptr()
        d.per_problem_stride = 4
        ctx = _context(0)
        g = torch.empty_like(x)
        capi.check(ctx._lib.mi355_check_derivatives_batch(ctx.handle, C.byref(d), None, 2, x.data_ptr(), None,
                                                          g.data_ptr(), None, None, None, None, None))
    assert e.value.code == -4 and "without LDS data" in str(e.value)
    svm = amd.Context(0, library=os.path.join(T.REPO, "cppnumericalsolvers_amd", "libmi355_lbfgs_svm.so"))
    try:
        rc, msg = T.device_check(svm, 100, np.zeros((2, 8)), np.zeros(0), dv_cases.config(3), hessian=False, check=False)
        assert rc == -4 and "derivatives=True" in msg, (rc, msg)
    finally:
        svm.close()


def test_cpp_header_on_device():
    exe = os.path.join(T.DV_DIR, "_build", "dv_header_test")
    assert os.path.exists(exe), "build() makes tests/derivatives/_build/dv_header_test"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
