"""The listed mode of the ask/tell handles (mi355_ask_tell_compact_*, mi355_ask_tell_ids_*) without a GPU: its six
symbols are declared, exported and listed with argtypes; null arguments are argument errors and crash nothing; the header
test program compiles with plain g++ with and without exceptions; and, from the code-object metadata of a gfx950
cross-compile, the compaction kernels and the step kernels of the three paths, listed and unlisted, run without scratch or
spilled vector registers while the unlisted fp64 step kernels keep the register counts of
profiles/ask_tell_kernel_resources.txt."""
import ctypes as C
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from cppnumericalsolvers_amd import _build

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PROGRAM_DIR = os.path.join(HERE, "ask_tell_compact")
PROGRAM = os.path.join(PROGRAM_DIR, "atc_header_test.cc")
SYMBOLS = tuple("mi355_ask_tell_%s_%s" % (call, suffix) for call in ("compact", "ids")
                for suffix in ("lbfgs", "lbfgs_f32", "lbfgsb"))


def test_symbols_are_declared_exported_and_listed():
    from cppnumericalsolvers_amd import capi
    lib = capi.load()
    header = open(os.path.join(REPO, "include", "mi355_lbfgs.h")).read()
    declared = set(re.findall(r"\b(mi355_ask_tell_[a-z0-9_]+)\s*\(", header))
    assert declared == set(SYMBOLS)
    assert sorted(capi.ASK_TELL_COMPACT_SYMBOLS) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert name not in capi.EXPORTED_SYMBOLS, name   # (that list is the mi355_lbfgs* / bfgs / auglag names')
    assert lib.mi355_lbfgs_abi_version() == 9


def test_null_arguments_are_argument_errors():
    from cppnumericalsolvers_amd import capi
    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    listed, p = C.c_int64(-7), C.c_void_p()
    not_a_handle = C.c_void_p(16)   # never dereferenced: the null out-pointer is refused first
    for suffix in ("lbfgs", "lbfgs_f32", "lbfgsb"):
        compact = getattr(lib, "mi355_ask_tell_compact_" + suffix)
        ids = getattr(lib, "mi355_ask_tell_ids_" + suffix)
        assert compact(None, C.byref(listed), None) == bad
        assert "null" in lib.mi355_lbfgs_last_error().decode()
        assert compact(None, None, None) == bad
        assert compact(not_a_handle, None, None) == bad
        assert ids(None, C.byref(p), C.byref(listed)) == bad
        assert ids(not_a_handle, None, C.byref(listed)) == bad
        assert ids(not_a_handle, C.byref(p), None) == bad
    assert listed.value == -7 and not p.value


@pytest.mark.parametrize("flags", [(), ("-fno-exceptions",)], ids=["plain", "fno-exceptions"])
def test_header_program_compiles(flags):
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", *flags,
                          "-I" + os.path.join(REPO, "include"), PROGRAM], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    text = open(PROGRAM).read()
    assert "MinimizeBatchWithCompaction" in text and "Compact()" in text and "Ids()" in text


# ---- the kernels' registers, from the metadata of a cross-compile -------------------------------------------------------
# unit -> {kernel name: how many instantiations the unit holds}
UNITS = {
    "dispatch_lbfgs_ask_tell": {"ask_tell::step_kernel": 6},
    "dispatch_lbfgs_ask_tell_listed": {"ask_tell::listed_step_kernel": 6},
    "dispatch_lbfgs_ask_tell_f32": {"ask_tell_f32::step_kernel": 6},
    "dispatch_lbfgs_ask_tell_f32_listed": {"ask_tell_f32::listed_step_kernel": 6},
    "dispatch_lbfgsb_ask_tell": {"ask_tell_box::step_kernel": 6},
    "dispatch_lbfgsb_ask_tell_listed": {"ask_tell_box::listed_step_kernel": 6},
    "dispatch_ask_tell_compact": {"ask_tell_compact::count_kernel": 3, "ask_tell_compact::scan_kernel": 1,
                                  "ask_tell_compact::scatter_kernel": 3},
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
        rows[field("name")] = dict(vgpr=int(field("vgpr_count")), vgpr_spill=int(field("vgpr_spill_count")),
                                   scratch=int(field("private_segment_fixed_size")))
    names = sorted(rows)
    demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(demangled) == len(names)
    return {re.sub(r"^void ", "", d).replace("mi355::", ""): rows[n] for n, d in zip(names, demangled)}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    out_dir = str(tmp_path_factory.mktemp("ask_tell_compact"))
    with ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        return dict(zip(UNITS, pool.map(lambda unit: _kernels(unit, out_dir), UNITS)))


def _of(rows, kernel):
    return {name: row for name, row in rows.items() if name.startswith(kernel + "<") or name.startswith(kernel + "(")}


@pytest.mark.parametrize("unit", [u for u in sorted(UNITS) if u != "dispatch_lbfgs_ask_tell"])
def test_new_kernels_run_without_scratch_or_spilled_vector_registers(compiled, unit):
    for kernel, count in UNITS[unit].items():
        rows = _of(compiled[unit], kernel)
        for name, row in sorted(rows.items()):
            print(name, row)
        assert len(rows) == count, (kernel, sorted(compiled[unit]))
        for name, row in rows.items():
            assert row["scratch"] == 0 and row["vgpr_spill"] == 0, (name, row)


def test_unlisted_step_kernels_keep_their_registers(compiled):
    """the figures of profiles/ask_tell_kernel_resources.txt, read from that file"""
    text = open(os.path.join(REPO, "profiles", "ask_tell_kernel_resources.txt")).read()
    want = {(int(w), int(e)): int(v) for w, e, v in re.findall(r"ask_tell::step_kernel<(\d+), (\d+)>\s+(\d+)\s", text)}
    assert want == {(8, 1): 124, (16, 1): 124, (32, 1): 124, (64, 1): 123, (64, 2): 134, (64, 4): 154}
    rows = _of(compiled["dispatch_lbfgs_ask_tell"], "ask_tell::step_kernel")
    assert len(rows) == 6, sorted(compiled["dispatch_lbfgs_ask_tell"])
    got = {}
    for name, row in rows.items():
        w, e = re.match(r"ask_tell::step_kernel<(\d+), (\d+)>", name).groups()
        got[(int(w), int(e))] = row["vgpr"]
        assert row["scratch"] == 0 and row["vgpr_spill"] == 0, (name, row)
    assert got == want
