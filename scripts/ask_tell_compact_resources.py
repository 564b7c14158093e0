"""Writes profiles/ask_tell_compact_resources.txt: the registers, scratch and LDS of the kernels the listed mode of the
ask/tell handles adds — the listed step kernels of the three paths and the compaction kernels — and, beside
them, of the unlisted step kernels they must leave as they were.  Read from the code-object metadata of a gfx950
cross-compile of the units (-S --cuda-device-only, the flags of _build.py): no GPU is needed.

    python scripts/ask_tell_compact_resources.py
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cppnumericalsolvers_amd import _build  # noqa: E402

UNITS = ("dispatch_lbfgs_ask_tell", "dispatch_lbfgs_ask_tell_listed", "dispatch_lbfgs_ask_tell_f32",
         "dispatch_lbfgs_ask_tell_f32_listed", "dispatch_lbfgsb_ask_tell", "dispatch_lbfgsb_ask_tell_listed",
         "dispatch_ask_tell_compact")


def kernels(unit, out_dir):
    """{demangled kernel name: dict(vgpr, agpr, sgpr, vgpr_spill, scratch, lds)} of one unit"""
    out = os.path.join(out_dir, unit + ".s")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "--offload-compress")]
    subprocess.check_call([_build.hipcc_path()] + flags + ["-I", _build.CSRC, "-S", "--cuda-device-only",
                                                           os.path.join(_build.CSRC, unit + ".hip"), "-o", out])
    rows = {}
    for block in open(out).read().split("- .agpr_count:")[1:]:
        def field(name):
            return re.search(r"\.%s:\s+(\S+)" % name, block).group(1)
        rows[field("name")] = dict(vgpr=int(field("vgpr_count")), agpr=int(block.split()[0]), sgpr=int(field("sgpr_count")),
                                   vgpr_spill=int(field("vgpr_spill_count")),
                                   scratch=int(field("private_segment_fixed_size")),
                                   lds=int(field("group_segment_fixed_size")))
    names = list(rows)
    demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return {short(d): rows[n] for n, d in zip(names, demangled)}


def short(demangled):
    """void mi355::ask_tell::step_kernel<8, 1>(mi355::ask_tell::Args) -> ask_tell::step_kernel<8, 1>"""
    name = re.sub(r"^void ", "", demangled)
    depth, end = 0, len(name)
    for i, ch in enumerate(name):   # cut the parameter list: the first '(' outside template brackets
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            end = i
            break
    name = name[:end].replace("mi355::", "")
    return re.sub(r"\(mi355::ask_tell(?:_f32|_box)?::Phase\)", "", name)


def main():
    with tempfile.TemporaryDirectory() as out_dir, ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        per_unit = dict(zip(UNITS, pool.map(lambda u: kernels(u, out_dir), UNITS)))
    lines = [
        "Resources of the kernels of the listed mode of the ask/tell handles (DESIGN.md 4.15), per unit of csrc/, beside the",
        "unlisted step kernels they leave as they were.  Read from the code-object metadata of a gfx950 cross-compile",
        "(hipcc " + " ".join(f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "--offload-compress")) +
        " -S --cuda-device-only;",
        "scripts/ask_tell_compact_resources.py writes this file).  VGPR: the metadata's vgpr_count, the AGPRs of the next",
        "column included (the Lbfgsb kernels that fill the 256 VGPRs).  LDS: the static part (the Lbfgsb step kernels add",
        "their dynamic layout, profiles/ask_tell_box_kernel_resources.txt).  The instructions of the unlisted step kernels are",
        "those of the units before the listed mode existed, compared function by function on this output.",
        "",
    ]
    width = max(len(name) for rows in per_unit.values() for name in rows)
    for unit in UNITS:
        lines.append("%s.hip" % unit)
        lines.append("  %-*s  VGPR  AGPR  SGPR  spilled VGPRs  scratch  static LDS" % (width, "kernel"))
        for name, r in sorted(per_unit[unit].items()):
            lines.append("  %-*s  %4d  %4d  %4d  %13d  %5d B  %8d B" % (width, name, r["vgpr"], r["agpr"], r["sgpr"],
                                                                          r["vgpr_spill"], r["scratch"], r["lds"]))
        lines.append("")
    path = os.path.join(ROOT, "profiles", "ask_tell_compact_resources.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
