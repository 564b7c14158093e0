"""Writes profiles/ask_tell_wide_kernel_resources.txt: the registers, scratch and LDS of the kernels of the ask/tell
L-BFGS path above n = 256 — the step kernels for 256 and 1024 threads per problem, dense and listed,
the workgroup evaluation of the built-in objectives, the state initialisation, the result gather and the path's
compaction kernels.  Read from the code-object metadata of a gfx950 cross-compile of the two units, the instructions
counted on the same listing (scripts/ask_tell_compact_resources.py has the reader): no GPU is needed.

    python scripts/ask_tell_wide_resources.py
"""
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cppnumericalsolvers_amd import _build  # noqa: E402
from ask_tell_compact_resources import kernels  # noqa: E402

UNITS = ("dispatch_lbfgs_ask_tell_wide", "dispatch_lbfgs_ask_tell_wide_listed")


def main():
    with tempfile.TemporaryDirectory() as out_dir, ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        per_unit = dict(zip(UNITS, pool.map(lambda u: kernels(u, out_dir), UNITS)))
    lines = [
        "Resources of the kernels of the ask/tell L-BFGS path above n = 256 (DESIGN.md 4.16), per unit of csrc/.  Read from the",
        "code-object metadata of a gfx950 cross-compile (hipcc " +
        " ".join(f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "--offload-compress")) + " -S --cuda-device-only;",
        "scripts/ask_tell_wide_resources.py writes this file).  LDS: the static part; a step kernel adds n rounded up to even",
        "doubles of dynamic LDS while the direction lives there (n <= 4096: at most 32 KB).  A 1024-thread workgroup has 128",
        "registers a thread.  Instructions: counted on the same listing.",
        "",
    ]
    width = max(len(name) for rows in per_unit.values() for name in rows)
    for unit in UNITS:
        lines.append("%s.hip" % unit)
        lines.append("  %-*s  VGPR  AGPR  SGPR  spilled VGPRs  scratch  static LDS  instructions" % (width, "kernel"))
        for name, r in sorted(per_unit[unit].items()):
            lines.append("  %-*s  %4d  %4d  %4d  %13d  %5d B  %8d B  %12d" % (width, name, r["vgpr"], r["agpr"], r["sgpr"],
                                                                             r["vgpr_spill"], r["scratch"], r["lds"],
                                                                             r["instructions"]))
        lines.append("")
    path = os.path.join(ROOT, "profiles", "ask_tell_wide_kernel_resources.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
