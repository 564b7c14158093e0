"""Writes profiles/ask_tell_compact_resources.txt: the registers, scratch and LDS of the kernels the listed mode of the
ask/tell handles adds — the listed step kernels of the three paths and the compaction kernels — and, beside
them, of the unlisted step kernels, which are entry points of the same run_steps.  Read from the code-object metadata of
a gfx950 cross-compile of the units (-S --cuda-device-only, the flags of _build.py), the instructions counted on the same
listing: no GPU is needed.  --before DIR: a csrc/ directory of another commit; its registers and instructions are
written beside each kernel it also holds.

    python scripts/ask_tell_compact_resources.py [--before <other checkout>/cppnumericalsolvers_amd/csrc --before-commit <hash>]
"""
import argparse
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


def kernels(unit, out_dir, csrc=_build.CSRC):
    """{demangled kernel name: dict(vgpr, agpr, sgpr, vgpr_spill, scratch, lds, instructions)} of one unit"""
    out = os.path.join(out_dir, unit + ".s")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "--offload-compress")]
    subprocess.check_call([_build.hipcc_path()] + flags + ["-I", csrc, "-S", "--cuda-device-only",
                                                           os.path.join(csrc, unit + ".hip"), "-o", out])
    text = open(out).read()
    rows = {}
    for block in text.split("- .agpr_count:")[1:]:
        def field(name):
            return re.search(r"\.%s:\s+(\S+)" % name, block).group(1)
        rows[field("name")] = dict(vgpr=int(field("vgpr_count")), agpr=int(block.split()[0]), sgpr=int(field("sgpr_count")),
                                   vgpr_spill=int(field("vgpr_spill_count")),
                                   scratch=int(field("private_segment_fixed_size")),
                                   lds=int(field("group_segment_fixed_size")))
    lines = text.split("\n")
    for name, row in rows.items():   # instructions: from the kernel's label to the end of its function
        start = next(i for i, line in enumerate(lines) if line.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        row["instructions"] = sum(1 for line in lines[start + 1:end] if re.match(r"\t[a-z]", line))
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", default=None, help="csrc/ of another commit to set beside")
    ap.add_argument("--before-commit", default="another commit", help="how the file names that commit (its hash)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as out_dir, ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        per_unit = dict(zip(UNITS, pool.map(lambda u: kernels(u, out_dir), UNITS)))
    before = {}
    if args.before:
        with tempfile.TemporaryDirectory() as out_dir, ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
            before = dict(zip(UNITS, pool.map(lambda u: kernels(u, out_dir, os.path.abspath(args.before)), UNITS)))
    lines = [
        "Resources of the kernels of the listed mode of the ask/tell handles (DESIGN.md 4.15), per unit of csrc/, beside the",
        "unlisted step kernels (the same run_steps without a list).  Read from the code-object metadata of a gfx950 cross-compile",
        "(hipcc " + " ".join(f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "--offload-compress")) +
        " -S --cuda-device-only;",
        "scripts/ask_tell_compact_resources.py writes this file).  VGPR: the metadata's vgpr_count, the AGPRs of the next",
        "column included (the Lbfgsb kernels that fill the 256 VGPRs).  LDS: the static part (the Lbfgsb step kernels add",
        "their dynamic layout, profiles/ask_tell_box_kernel_resources.txt).  Instructions: counted on the same listing.",
    ]
    if before:
        lines.append("before: VGPR / AGPR / instructions of the same kernel in commit %s, where every step kernel spelled the" % args.before_commit)
        lines.append("More-Thuente search and the grid loop out itself (now MtSearch, csrc/more_thuente_device.hpp, and run_steps).")
    lines.append("")
    width = max(len(name) for rows in per_unit.values() for name in rows)
    for unit in UNITS:
        lines.append("%s.hip" % unit)
        lines.append("  %-*s  VGPR  AGPR  SGPR  spilled VGPRs  scratch  static LDS  instructions%s"
                     % (width, "kernel", "  before" if before else ""))
        for name, r in sorted(per_unit[unit].items()):
            line = "  %-*s  %4d  %4d  %4d  %13d  %5d B  %8d B  %12d" % (width, name, r["vgpr"], r["agpr"], r["sgpr"],
                                                                          r["vgpr_spill"], r["scratch"], r["lds"],
                                                                          r["instructions"])
            b = before.get(unit, {}).get(name)
            if b:
                line += "  %d / %d / %d" % (b["vgpr"], b["agpr"], b["instructions"])
            lines.append(line)
        lines.append("")
    path = os.path.join(ROOT, "profiles", "ask_tell_compact_resources.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
