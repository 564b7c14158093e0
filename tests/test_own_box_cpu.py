"""One box per problem (SetBoundsPerProblem, mi355_lbfgsb_minimize_batch_boxes) — what is checked without a GPU.

1. The inputs of tests/own_box_cases.py exercise the box: per case, from the per-box oracle results alone.
2. Register budget of the kernels that read the box per problem, against their shared-box twins: gfx950 cross-compiles
   of the two new units and of the units that hold the twins (code-object metadata; no GPU needed).
3. The drop-in header: the overload exists next to the old ones, compiles with and without exceptions, and refuses a
   size mismatch, a dimension mismatch and a NaN through Fail before it reaches the library.
"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import own_box_cases as cases
from cppnumericalsolvers_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["default", "parity"])
@pytest.mark.parametrize("name", [c["name"] for c in cases.CASES])
def test_inputs_exercise_the_box(oracle, name, preset):
    x, f, g, p = cases.twin(oracle, name, preset)
    x0, lower, upper, _ = cases.inputs(cases.BY_NAME[name])
    assert np.isfinite(x).all() and np.isfinite(f).all() and np.isfinite(g).all()
    for k in ("x_delta", "f_delta", "gradient_norm"):
        assert np.isfinite(p[k]).all(), k
    assert ((x >= lower) & (x <= upper)).all()
    on_bound = ((x == lower) | (x == upper)).any(axis=1)
    pairs = set(zip(p["status"].tolist(), p["num_iterations"].tolist()))
    print("%s %s: %d of %d rows end on a bound, %d status / iteration pairs, iterations %d..%d" %
          (name, preset, on_bound.sum(), cases.B, len(pairs), p["num_iterations"].min(), p["num_iterations"].max()))
    assert on_bound.sum() * 4 >= cases.B
    assert (~on_bound).sum() * 8 >= cases.B
    assert len(pairs) >= 3
    which = cases.box_of_row()
    assert (x0[which == 7] < lower[which == 7]).all()                     # box 8: the projection moves the whole point
    half = (x0[which == 8] == lower[which == 8]) | (x0[which == 8] == upper[which == 8])
    assert (half.sum(axis=1) == (cases.BY_NAME[name]["n"] + 1) // 2).all()   # box 9: half the coordinates start on a bound


# ---- 2. registers -----------------------------------------------------------------------------------------------------
SHARED_UNITS = ("dispatch_lbfgsb", "dispatch_lbfgsb_e4", "dispatch_lbfgsb_fast")
OWN_UNITS = ("dispatch_lbfgsb_own_box", "dispatch_lbfgsb_fast_own_box")
PLAIN = ("mi355::RosenbrockObjectiveT<false>", "mi355::DiagQuadraticObjective<%d>")


def _expected_own_box_kernels():
    """Template arguments (without the trailing OwnBox) of the kernels the two units are to hold."""
    exact, relaxed = set(), set()
    for E in (1, 2, 4):
        for obj in PLAIN:
            for M in (5, 8):
                exact.add("lbfgsb_solve_kernel<%d, %s, %d, 0, mi355::NoOuterLoop, 16" % (E, obj % E if "%d" in obj else obj, M))
        exact.add("lbfgsb_solve_kernel<%d, mi355::SquaredErrorRidgeObjective<16, %d>, 5, 0, mi355::NoOuterLoop, 16" % (E, E))
    for E in (1, 2):
        for obj in PLAIN:
            for M in (5, 8):
                relaxed.add("lbfgsb_fast_kernel<%d, %s, %d, 16" % (E, obj % E if "%d" in obj else obj, M))
    return {"dispatch_lbfgsb_own_box": exact, "dispatch_lbfgsb_fast_own_box": relaxed}


def _waves_asked_for(key):
    """The second argument of the kernel's __launch_bounds__ (csrc/lbfgsb_kernel.hpp, csrc/lbfgsb_fast_kernel.hpp)."""
    E = int(re.match(r"\w+<(\d+),", key).group(1))
    M, W = (int(v) for v in re.search(r", (\d+), (?:0, mi355::NoOuterLoop, )?(\d+)$", key).groups())
    if key.startswith("lbfgsb_solve_kernel"):
        return 1 if (E >= 4 or M > 5 or W > 16) else 2
    return 1 if (M > 5 or E >= 8) else 2


def _kernels(unit, out_dir):
    out = os.path.join(out_dir, unit + ".s")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "--offload-compress")]
    subprocess.check_call([_build.hipcc_path()] + flags + ["-I", _build.CSRC, "-S", "--cuda-device-only",
                                                           os.path.join(_build.CSRC, unit + ".hip"), "-o", out])
    rows = {}
    for block in open(out).read().split("- .agpr_count:")[1:]:
        def field(name):
            return re.search(r"\.%s:\s+(\S+)" % name, block).group(1)
        rows[field("name")] = dict(vgpr=int(field("vgpr_count")), sgpr_spill=int(field("sgpr_spill_count")),
                                   vgpr_spill=int(field("vgpr_spill_count")),
                                   scratch=int(field("private_segment_fixed_size")),
                                   lds=int(field("group_segment_fixed_size")))
    names = list(rows)
    filt = os.path.join(os.path.dirname(os.path.realpath(_build.hipcc_path())), "..", "llvm", "bin", "llvm-cxxfilt")
    plain = subprocess.run([filt if os.path.exists(filt) else "c++filt"] + names, capture_output=True, text=True,
                           check=True).stdout.split("\n")
    out_rows = {}
    for mangled, text in zip(names, plain):
        m = re.match(r"void mi355::(lbfgsb_\w+_kernel<.*), (true|false)>\(", text)
        if m:   # (a unit may hold other kernels; none of these does)
            out_rows[(m.group(1), m.group(2) == "true")] = rows[mangled]
    assert len(out_rows) == len(rows), sorted(plain)
    return out_rows


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out_dir = str(tmp_path_factory.mktemp("own_box"))
    units = SHARED_UNITS + OWN_UNITS
    with ThreadPoolExecutor(max_workers=len(units)) as pool:
        return dict(zip(units, pool.map(lambda unit: _kernels(unit, out_dir), units)))


@pytest.mark.parametrize("unit", OWN_UNITS)
def test_own_box_units_hold_the_listed_kernels_within_the_budget_of_their_twins(compiled, unit):
    rows = compiled[unit]
    shared = {}
    for u in SHARED_UNITS:
        shared.update({key: row for (key, own), row in compiled[u].items() if not own})
    assert all(own for _, own in rows), sorted(rows)
    assert {key for key, _ in rows} == _expected_own_box_kernels()[unit], sorted(rows)
    for (key, _), row in sorted(rows.items()):
        twin = shared[key]
        print(key, "own box", row, "shared box", twin)
        if twin["scratch"] == 0:
            assert row["scratch"] == 0, (key, row)
        if twin["vgpr_spill"] == 0:
            assert row["vgpr_spill"] == 0, (key, row)
        assert row["vgpr"] <= 512 // _waves_asked_for(key), (key, row)     # 512 registers per SIMD lane on gfx950
        assert row["lds"] == twin["lds"], (key, row, twin)


# ---- 3. the drop-in header --------------------------------------------------------------------------------------------
HEADER_USE = r'''
#include <vector>
#include "cppoptlib/function.h"
#include "cppoptlib/solver/lbfgsb.h"
using F = cppoptlib::function::Rosenbrock<>;
using Solver = cppoptlib::solver::Lbfgsb<F>;
int main() {
  F f;
  Solver solver;
  std::vector<Solver::StateType> states;
  std::vector<F::VectorType> lower, upper;
  std::vector<F> functions;
#ifdef WITH_BOXES
  auto r = solver.MinimizeBatch(f, states, lower, upper);
#else
  solver.SetBounds(F::VectorType(2), F::VectorType(2));
  auto r = solver.MinimizeBatch(f, states);
  auto q = solver.MinimizeBatch(functions, states);
  (void)q;
#endif
  static_assert(std::is_same<decltype(r), std::vector<std::tuple<Solver::StateType, Solver::ProgressType>>>::value, "");
  return static_cast<int>(r.size());
}
'''


@pytest.mark.parametrize("flags", [[], ["-DWITH_BOXES"], ["-DWITH_BOXES", "-fno-exceptions"]],
                         ids=["as-before", "with-boxes", "with-boxes-no-exceptions"])
def test_header_compiles(tmp_path, flags):
    p = tmp_path / "t.cc"
    p.write_text(HEADER_USE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        str(p)] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_overload_refuses_a_mismatch_and_a_nan_through_fail():
    """tests/own_box/own_box_header_test.cc, `refusals`: thrown by cppoptlib::mi355::Fail before any context exists."""
    exe = os.path.join(ROOT, "tests", "own_box", "_build", "own_box_header_test")
    assert os.path.exists(exe), "tests/own_box/_build/own_box_header_test is missing: run __graft_entry__.build()"
    r = subprocess.run([exe, "refusals"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
