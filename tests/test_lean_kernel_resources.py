"""Register budget of the lean solve kernels (csrc/dispatch_lean.hip), read from the code-object metadata of a gfx950
cross-compile (no GPU needed).  The general kernel's figures come from the same compile — a probe unit that instantiates
it next to the lean unit — not from a constant."""
import os
import re
import subprocess

from cppnumericalsolvers_amd import _build

PROBE = """#define MI355_DISPATCH_TU 1
#include "engine_internal.hpp"
namespace mi355 {
int general_w8(mi355_lbfgs_ctx* ctx, const SolveArgs& args, hipStream_t stream) {
  return launch_solve<8, 4, RosenbrockFullObjective, 6, MI355_LS_MORE_THUENTE, kAlgLbfgs, NoOuterLoop, ArithFma>(ctx, args, stream);
}
int general_w16(mi355_lbfgs_ctx* ctx, const SolveArgs& args, hipStream_t stream) {
  return launch_solve<16, 4, RosenbrockFullObjective, 10, MI355_LS_MORE_THUENTE, kAlgLbfgs, NoOuterLoop, ArithFma>(ctx, args, stream);
}
}  // namespace mi355
"""


def _kernels(source, out):
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "--offload-compress")]
    subprocess.check_call([_build.hipcc_path()] + flags + ["-I", _build.CSRC, "-S", "--cuda-device-only", source, "-o", out])
    text = open(out).read()
    rows = {}
    for block in text.split("- .agpr_count:")[1:]:
        def field(name):
            return re.search(r"\.%s:\s+(\S+)" % name, block).group(1)
        rows[field("name")] = dict(vgpr=int(field("vgpr_count")), sgpr_spill=int(field("sgpr_spill_count")),
                                   vgpr_spill=int(field("vgpr_spill_count")),
                                   scratch=int(field("private_segment_fixed_size")))
    return rows


def _only(rows, W, MR):
    key = "lbfgs_solve_kernelILi%dELi4E" % W
    hits = [v for k, v in rows.items() if key in k and "ELi%dELi0ELi0E" % MR in k]
    assert len(hits) == 1, (W, MR, sorted(rows))
    return hits[0]


def test_lean_unit_holds_four_kernels_with_smaller_budgets(tmp_path):
    probe = tmp_path / "general_probe.hip"
    probe.write_text(PROBE)
    general = _kernels(str(probe), str(tmp_path / "general_probe.s"))
    lean = _kernels(os.path.join(_build.CSRC, "dispatch_lean.hip"), str(tmp_path / "dispatch_lean.s"))
    assert len(lean) == 4 and all("lbfgs_solve_kernel" in k and "FixedOptions" in k for k in lean), sorted(lean)
    assert all("RunTimeOptions" in k for k in general) and len(general) == 2
    for W, MR in ((8, 6), (16, 10)):     # configs[1], configs[2]
        g, l = _only(general, W, MR), _only(lean, W, MR)
        print("W=%d MR=%d general %s lean %s" % (W, MR, g, l))
        assert l["scratch"] == 0 and l["vgpr_spill"] == 0
        assert l["vgpr"] <= g["vgpr"]
        assert l["sgpr_spill"] < g["sgpr_spill"]
    for row in lean.values():
        assert row["scratch"] == 0 and row["vgpr_spill"] == 0
