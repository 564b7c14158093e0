"""Register budget of the kernels built on csrc/solver_driver.hpp (TrustRegionNewton, NewtonDescent, NelderMead and the
first-order solvers), read from the code-object metadata of a gfx950 cross-compile of their four units (no GPU needed).
The shared pieces are __forceinline__ functions and a struct of scalars; a kernel with scratch or a spilled vector register
would mean the struct is no longer kept in registers."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from cppnumericalsolvers_amd import _build

# unit -> (the kernel's name, how many the unit holds: objectives x lane mappings (x modes / methods))
UNITS = {
    "dispatch_trust_region": ("trust_region_kernel", 2 * 4),
    "dispatch_newton_descent": ("newton_descent_kernel", 2 * 4),
    "dispatch_nelder_mead": ("nelder_mead_kernel", 2 * 4 * 2),
    "dispatch_first_order": ("first_order_kernel", 2 * 6 * 2),
}


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
                                   scratch=int(field("private_segment_fixed_size")))
    return rows


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out_dir = str(tmp_path_factory.mktemp("solver_driver"))
    with ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        return dict(zip(UNITS, pool.map(lambda unit: _kernels(unit, out_dir), UNITS)))


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_unit_holds_its_kernels_without_scratch_or_vector_spills(compiled, unit):
    kernel, count = UNITS[unit]
    rows = compiled[unit]
    for name, row in sorted(rows.items()):
        print(name, row)
    assert len(rows) == count and all(kernel in name for name in rows), sorted(rows)
    for name, row in rows.items():
        assert row["scratch"] == 0 and row["vgpr_spill"] == 0, (name, row)
