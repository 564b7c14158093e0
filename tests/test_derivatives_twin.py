"""The CPU twin of the derivative checker (tests/derivatives/dv_twin.hpp): in reference order bit for bit the reference's
unmodified utils/derivatives.h (the recorded outputs, and a fresh draw where the reference tree exists) and the repository's
own host header; the margin rule of the pass and planted cases in BOTH summation orders; planted errors caught at the
planted index; the NaN-passes rule and the nonfinite count; the distance between the two orders' finite differences."""
import os
import re
import subprocess

import numpy as np
import pytest

import dv_cases
import dv_lib as T

CASES = dv_cases.make_cases()
BY_NAME = {c["name"]: c for c in CASES}
GOLDEN = dv_cases.load_golden()
RECORDED = [c for c in CASES if c["name"] + "/grad_fd" in GOLDEN]
_twin_cache = {}


def _twin(case, order, hessian=None):
    key = (case["name"], order, hessian)
    if key not in _twin_cache:
        _twin_cache[key] = T.twin_check(case["objective"], case["x"], case["params"], case["config"], order=order,
                                        hessian=case["hessian"] if hessian is None else hessian)
    return _twin_cache[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _assert_twin_is(case, ref, what):
    tw = _twin(case, T.REF_ORDER, hessian=True)
    assert (_bits(tw["grad_fd"]) == _bits(ref["grad_fd"])).all(), (what, case["name"], "grad_fd")
    assert (tw["report"]["gradient_ok"] == ref["gradient_ok"]).all(), (what, case["name"], "gradient verdict")
    assert (tw["report"]["hessian_ok"] == ref["hessian_ok"]).all(), (what, case["name"], "Hessian verdict")
    if "hess_fd" in ref:
        assert (_bits(tw["hess_fd"]) == _bits(ref["hess_fd"])).all(), (what, case["name"], "hess_fd")
    else:
        assert dv_cases.digest(tw["hess_fd"]) == ref["hess_fd_sha256"], (what, case["name"], "hess_fd digest")


@pytest.mark.parametrize("case", RECORDED, ids=[c["name"] for c in RECORDED])
def test_twin_reference_order_matches_golden(case):
    name = case["name"]
    assert (_bits(GOLDEN[name + "/x"]) == _bits(case["x"])).all() and (_bits(GOLDEN[name + "/params"]) == _bits(case["params"])).all()
    ref = dict(grad_fd=GOLDEN[name + "/grad_fd"], gradient_ok=GOLDEN[name + "/gradient_ok"],
               hessian_ok=GOLDEN[name + "/hessian_ok"])
    if name + "/hess_fd" in GOLDEN:
        ref["hess_fd"] = GOLDEN[name + "/hess_fd"]
    else:
        ref["hess_fd_sha256"] = str(GOLDEN[name + "/hess_fd_sha256"])
    _assert_twin_is(case, ref, "golden")


def test_golden_file_covers_the_cases_and_stays_small():
    assert os.path.getsize(dv_cases.GOLDEN) < 1 << 20
    unrecorded = [c["name"] for c in CASES if c not in RECORDED]
    # only what the reference cannot run (a step override) or what would not fit (n > 64) is left out
    assert all(BY_NAME[n]["x"].shape[1] > 64 or BY_NAME[n]["config"]["hessian_step"] for n in unrecorded), unrecorded
    assert {c["x"].shape[1] for c in CASES if not c["hessian"]} >= set(dv_cases.GRADIENT_N)
    assert {c["x"].shape[1] for c in CASES if c["hessian"]} >= set(dv_cases.HESSIAN_N)
    assert {c["x"].shape[0] for c in CASES} == set(dv_cases.BATCHES)
    assert {c["config"]["gradient_accuracy"] for c in CASES if not c["hessian"]} == {0, 1, 2, 3}


@pytest.fixture(scope="module")
def reference_library(tmp_path_factory):
    if not os.path.isdir(T.REFERENCE):
        pytest.skip("needs the reference tree")
    return T.build_reference(str(tmp_path_factory.mktemp("dv_ref")))


def test_twin_matches_reference_on_every_recorded_case(reference_library):
    for case in RECORDED:
        _assert_twin_is(case, T.reference_check(reference_library, case["objective"], case["x"], case["params"],
                                                case["config"]), "reference")


def test_twin_matches_reference_fresh_draw(reference_library):
    rng = np.random.default_rng()
    seed = int(rng.integers(1 << 31))
    rng = np.random.default_rng(seed)
    for objective, n in ((T.ROSENBROCK, 7), (T.DIAG_QUADRATIC, 12), (T.QUARTIC, 3), (T.DENSE, 10), (T.PLANTED, 11)):
        x = rng.normal(size=(3, n)) * rng.choice([0.3, 2.0], size=(3, n))
        params = {T.DIAG_QUADRATIC: np.concatenate([rng.normal(size=n), [1.5]]),
                  T.DENSE: np.concatenate([rng.normal(size=n * n + n), [0.7]]),
                  T.PLANTED: dv_cases.planted_params(n, 3, 2, 5, 4.0)}.get(objective)
        for accuracy in range(4):
            case = dict(name="fresh_%d_%d_%d_seed%d" % (objective, n, accuracy, seed), objective=objective, x=x,
                        params=params if params is not None else np.zeros(1), config=dv_cases.config(accuracy),
                        hessian=True)
            _assert_twin_is(case, T.reference_check(reference_library, objective, x, case["params"], case["config"]),
                            "fresh draw")


MARGIN_CASES = [c for c in CASES if c["kind"] in ("pass", "planted")]


@pytest.mark.parametrize("case", MARGIN_CASES, ids=[c["name"] for c in MARGIN_CASES])
def test_margin_rule_and_verdicts(case):
    """A verdict that must pass has worst excess < 0.5, one that must fail > 2, in both summation orders: no expectation
    hinges on rounding.  Planted errors are caught, and the worst index is the planted one."""
    for order in (T.REF_ORDER, T.DEVICE_ORDER):
        rep = _twin(case, order)["report"]
        for which in (("gradient", "hessian") if case["hessian"] else ("gradient",)):
            excess = rep[which + "_worst_excess"]
            must_fail = case["kind"] == "planted" and (case["fails"] == which or case.get("other_fails"))
            if must_fail:
                assert (excess > 2.0).all() and (rep[which + "_ok"] == 0).all(), (order, which, rep)
            else:
                assert (excess < 0.5).all() and (rep[which + "_ok"] == 1).all(), (order, which, rep)
        if case["kind"] == "planted":
            got = rep[case["fails"] + "_worst_index"]
            if case["worst_index"] is not None:
                assert (got == case["worst_index"]).all(), (order, got)
            else:
                assert np.isin(got, case["worst_among"]).all(), (order, got)


def test_one_sided_plant_makes_the_functors_hessian_asymmetric():
    case = BY_NAME["planted_one_sided_n17_i08_j07"]
    out = _twin(case, T.DEVICE_ORDER)
    H, F = out["hess"][0], out["hess_fd"][0]
    assert (F == F.T).all() and H[7, 8] != H[8, 7] and H[7, 8] - H[8, 7] == 8.0   # [j, i] = H(i, j): H(8, 7) is planted
    assert (out["report"]["hessian_ok"] == 0).all()


def test_nan_passes_and_nonfinite_is_counted():
    for name in ("special_rosenbrock_n09", "special_rosenbrock_n09_a0"):
        case = BY_NAME[name]
        n = case["x"].shape[1]
        for order in (T.REF_ORDER, T.DEVICE_ORDER):
            out = _twin(case, order)
            rep = out["report"]
            # row 2 holds 1e200: f overflows to inf - inf, every finite-difference entry is NaN and every one passes
            assert np.isnan(out["grad_fd"][2]).all() and np.isnan(out["hess_fd"][2]).all()
            assert rep["gradient_ok"][2] == 1 and rep["hessian_ok"][2] == 1 and rep["nonfinite"][2] == n + n * n
            assert rep["gradient_worst_index"][2] == -1 and rep["gradient_worst_excess"][2] == 0.0
            # rows 0 and 3 hold a 0 and a -0: the step is sqrt(eps) * 1 there, nothing non-finite
            assert (rep["nonfinite"][[0, 1, 3, 4]] == 0).all() and np.isfinite(out["grad_fd"][[0, 3]]).all()
            # row 1 holds 2^40: h = 2^14 there, a finite difference over a step that wide is wrong and the check says so
            assert rep["gradient_ok"][1] == 0


def test_cross_order_distance_is_what_design_records():
    """How far the finite differences of the two summation orders lie apart, over all cases (the special points aside),
    in units of the rounding noise a difference of values carries: eps max(|f|, 1) / h for the gradient and
    eps max(|f|, 1) / h^2 for the Hessian, h the step factor (2^-26, or the override).  DESIGN.md 4.10 quotes the two
    figures; the bound a numerical comparison of the orders may use is 4 x them (margin for cases not drawn)."""
    eps = 2.0 ** -52
    worst_g = worst_h = 0.0
    for case in CASES:
        if case["name"].startswith("special"):
            continue
        a, b = _twin(case, T.REF_ORDER), _twin(case, T.DEVICE_ORDER)
        scale = np.maximum(np.abs(a["f"]), 1.0)
        hg = case["config"]["gradient_step"] or 2.0 ** -26
        worst_g = max(worst_g, float(np.max(np.abs(a["grad_fd"] - b["grad_fd"]) / (eps * scale[:, None] / hg))))
        if case["hessian"]:
            hh = case["config"]["hessian_step"] or 2.0 ** -26
            worst_h = max(worst_h, float(np.max(np.abs(a["hess_fd"] - b["hess_fd"]) / (eps * scale[:, None, None] / hh ** 2))))
    print("cross-order distance: gradient %.3g, Hessian %.3g noise units" % (worst_g, worst_h))
    design = open(os.path.join(T.REPO, "DESIGN.md")).read()
    m = re.search(r"cross-order distance: gradient ([0-9.e+-]+), Hessian ([0-9.e+-]+) noise units", design)
    assert m, "DESIGN.md 4.10 quotes the measured cross-order distance"
    assert worst_g <= 4.0 * float(m.group(1)) and worst_h <= 4.0 * float(m.group(2)), (worst_g, worst_h)


HOST_HEADER_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "cppoptlib/function.h"
#include "cppoptlib/utils/derivatives.h"
#include "common.h"
extern "C" int dv_twin_check(int, int, int64_t, const double*, const dv_config*, int, int, int, const double*, double*,
                             double*, double*, double*, double*, dv_report*);
using cppoptlib::function::DifferentiabilityMode;
using cppoptlib::function::FunctionCRTP;
class Rosenbrock : public FunctionCRTP<Rosenbrock, double, DifferentiabilityMode::First> {
 public:
  ScalarType operator()(const VectorType& x, VectorType* = nullptr) const {
    const int n = static_cast<int>(x.size());
    double f = 0.0;
    for (int i = 0; i + 1 < n; ++i) {
      const double t1 = 1.0 - x[i], t2 = x[i + 1] - x[i] * x[i];
      const double term = t1 * t1 + (100.0 * t2) * t2;
      f = (i == 0) ? term : f + term;
    }
    return f;
  }
};
int main() {
  const int n = 7;
  const double xs[n] = {0.3, -1.7, 0.0, 2.5, -0.4, 1.0009765625, 0.75};
  Rosenbrock f;
  Rosenbrock::VectorType x(n);
  for (int i = 0; i < n; ++i) x[i] = xs[i];
  int bad = 0;
  for (int accuracy = 0; accuracy < 4; ++accuracy) {
    dv_config c{accuracy, accuracy, 0, 0, 0, 0};
    double tf, tg[n], tgfd[n], th[n * n], thfd[n * n];
    dv_report r;
    if (dv_twin_check(kDvRosenbrock, n, 1, nullptr, &c, 0, 8, 1, xs, &tf, tg, tgfd, th, thfd, &r) != 0) return 2;
    Rosenbrock::VectorType g;
    cppoptlib::utils::ComputeFiniteGradient(f, x, &g, accuracy);
    cppoptlib::mi355::SquareMatrix<double, cppoptlib::function::kDynamicDimension> H;
    cppoptlib::utils::ComputeFiniteHessian(f, x, &H, accuracy);
    for (int i = 0; i < n; ++i) bad += std::memcmp(&g[i], &tgfd[i], 8) != 0;
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i) {
        const double v = H(i, j);
        bad += std::memcmp(&v, &thfd[j * n + i], 8) != 0;
      }
  }
  std::printf("%d\n", bad);
  return bad != 0;
}
"""


def test_twin_matches_the_repositorys_host_header(tmp_path):
    """cppoptlib::utils::ComputeFiniteGradient / ComputeFiniteHessian of include/ (the host-side checks) on a point whose
    values are all positive, so that a sum begun at 0 and one begun at its first term agree: bit for bit the twin."""
    src = tmp_path / "host_header.cc"
    src.write_text(HOST_HEADER_PROGRAM)
    exe = str(tmp_path / "host_header")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(T.REPO, "include"),
                           "-I" + T.DV_DIR, str(src), "-L" + os.path.dirname(T.TWIN_LIB), "-ldv_twin",
                           "-Wl,-rpath," + os.path.dirname(T.TWIN_LIB), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


def test_c_abi_config_defaults_and_symbols():
    import ctypes as C
    from cppnumericalsolvers_amd import capi
    c = capi.default_derivative_config()
    assert (c.gradient_accuracy, c.hessian_accuracy) == (3, 3)
    assert (c.gradient_step, c.hessian_step, c.gradient_tolerance, c.hessian_tolerance) == (0.0, 0.0, 0.0, 0.0)
    assert capi.default_derivative_config(hessian_step=2.0 ** -13).hessian_step == 2.0 ** -13
    with pytest.raises(TypeError):
        capi.default_derivative_config(rho=0.5)
    assert C.sizeof(capi.DerivativeConfig) == T.CONFIG_DTYPE.itemsize == 40
    assert capi.DERIVATIVE_REPORT_DTYPE == T.REPORT_DTYPE
    lib = capi.load()
    header = open(os.path.join(T.REPO, "include", "mi355_lbfgs.h")).read()
    declared = sorted(set(re.findall(r"\b(mi355_(?:derivative|check_derivatives)_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(capi.DERIVATIVE_SYMBOLS)
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert lib.mi355_lbfgs_abi_version() == 9


def test_build_recipe_generates_one_derivative_unit(tmp_path):
    from cppnumericalsolvers_amd import _build
    header = os.path.join(T.DV_DIR, "planted.hpp")
    paths = _build.user_objective_sources([dict(name="planted", type="dv_test::Planted", id=102, lbfgs=False, lbfgsb=False,
                                                derivatives=dict(elems=(1, 2)), header=header)], str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ["user_planted_derivatives.hip"]
    text = open(paths[0]).read()
    assert "UserDerivativesRegistration registration_102_derivatives" in text and "derivative_check_launch.hpp" in text
    assert text.count("using type = dv_test::Planted;") == 5 and text.count("using type = DerivativeNotBuilt;") == 1
    for name in ("dispatch_derivatives.hip",):
        assert name in _build.SOURCES
    for name in ("derivative_check_kernel.hpp", "derivative_check_config.hpp", "derivative_check_launch.hpp"):
        assert name in _build.HEADERS
