"""The kernels of the ask/tell L-BFGS path above n = 256, from the code-object metadata of a gfx950 cross-compile of its
two units (no GPU): the expected kernels are there, each runs without scratch and without spilled vector registers —
the 1024-thread step kernels included, which have 128 registers a thread — and profiles/ask_tell_wide_kernel_resources.txt
lists every one of them."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from cppnumericalsolvers_amd import _build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# unit -> {kernel name: how many instantiations the unit holds}
UNITS = {
    "dispatch_lbfgs_ask_tell_wide": {"ask_tell_wide::step_kernel": 2, "ask_tell_wide::eval_kernel": 4,
                                     "ask_tell_common::init_kernel": 1, "ask_tell_common::results_kernel": 1},
    "dispatch_lbfgs_ask_tell_wide_listed": {"ask_tell_wide::listed_step_kernel": 2, "ask_tell_compact::count_kernel": 1,
                                            "ask_tell_compact::scan_kernel": 1, "ask_tell_compact::scatter_kernel": 1},
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
        rows[field("name")] = dict(vgpr=int(field("vgpr_count")), sgpr=int(field("sgpr_count")),
                                   vgpr_spill=int(field("vgpr_spill_count")), sgpr_spill=int(field("sgpr_spill_count")),
                                   lds=int(field("group_segment_fixed_size")),
                                   scratch=int(field("private_segment_fixed_size")),
                                   threads=int(field("max_flat_workgroup_size")))
    names = sorted(rows)
    demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(demangled) == len(names)
    return {re.sub(r"^void ", "", d).replace("mi355::", ""): rows[n] for n, d in zip(names, demangled)}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out_dir = str(tmp_path_factory.mktemp("ask_tell_wide"))
    with ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        return dict(zip(UNITS, pool.map(lambda unit: _kernels(unit, out_dir), UNITS)))


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_kernels_run_without_scratch_or_spilled_vector_registers(compiled, unit):
    assert sum(UNITS[unit].values()) == len(compiled[unit]), sorted(compiled[unit])
    for kernel, count in UNITS[unit].items():
        rows = {name: row for name, row in compiled[unit].items() if name.startswith(kernel + "<")}
        for name, row in sorted(rows.items()):
            print(name, row)
        assert len(rows) == count, (kernel, sorted(compiled[unit]))
        for name, row in rows.items():
            assert row["scratch"] == 0 and row["vgpr_spill"] == 0, (name, row)


def test_step_kernels_are_built_for_256_and_1024_threads(compiled):
    for unit, kernel in (("dispatch_lbfgs_ask_tell_wide", "ask_tell_wide::step_kernel"),
                         ("dispatch_lbfgs_ask_tell_wide_listed", "ask_tell_wide::listed_step_kernel")):
        got = {int(re.match(re.escape(kernel) + r"<(\d+)>", name).group(1)): row
               for name, row in compiled[unit].items() if name.startswith(kernel + "<")}
        assert sorted(got) == [256, 1024]
        for T, row in got.items():
            assert row["threads"] == T
            assert row["vgpr"] <= 128 or T == 256, (T, row)   # sixteen wavefronts of a workgroup share a CU's four SIMDs


def test_the_committed_table_lists_every_kernel(compiled):
    """profiles/ask_tell_wide_kernel_resources.txt (scripts/ask_tell_wide_resources.py): a row per kernel, named without
    its parameter list, with the registers, scratch and static LDS of this compile"""
    text = open(os.path.join(REPO, "profiles", "ask_tell_wide_kernel_resources.txt")).read()
    for unit in UNITS:
        for name, row in compiled[unit].items():
            short = name[:name.index(">(") + 1]
            found = re.findall(r"^  %s\s+(\d+)\s+\d+\s+\d+\s+(\d+)\s+(\d+) B\s+(\d+) B\s+\d+$" % re.escape(short), text, re.M)
            assert len(found) == 1, short
            assert tuple(int(v) for v in found[0]) == (row["vgpr"], row["vgpr_spill"], row["scratch"], row["lds"]), (short, row)
