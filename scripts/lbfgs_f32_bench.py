"""Native fp32 L-BFGS against the fp64 exact kernel on the same starts (needs an MI355X).

Two shapes: BASELINE.json configs[1] (65,536 x Rosenbrock-32, m = 6) and a configs[2]-shaped batch (Rosenbrock-64,
m = 10).  Stopping: the reference's default preset for both precisions — the thresholds of parity_stop() sit below float
resolution.  In one process, alternating float / double for `--rounds` rounds after a warm-up of each: the float entry
(mi355_lbfgs_minimize_batch_f32) and the fp64 kernel with MI355_ARITH_EXACT and MI355_HISTORY_LDS on the widened starts.
Per round and precision one JSON line goes to profiles/lbfgs_f32_bench.jsonl (or --out): solves/s over the kernel time
(device events around the launch, mi355_lbfgs_last_kernel_ms), kernel ms, the batch's total num_iterations and kernel
ms per problem-iteration (kernel time / sum of num_iterations); a summary line per shape carries the medians and the
ratio float / double of the per-problem-iteration medians.  No figure is asserted.
    python scripts/lbfgs_f32_bench.py [--rounds 5] [--batch2 131072] [--out profiles/lbfgs_f32_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def run(solver, objective, x0, amd, torch):
    x, f, g, p = solver.minimize(objective, x0)
    torch.cuda.synchronize()
    ms = solver.last_kernel_ms()
    prog = amd.progress_to_numpy(p)
    return ms, int(prog["num_iterations"].sum()), prog, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch2", type=int, default=131072, help="problems of the configs[2]-shaped batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbfgs_f32_bench.jsonl"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi

    ctx = amd.Context(0)
    shapes = [dict(name="configs[1]", B=65536, n=32, m=6), dict(name="configs[2]-shaped", B=args.batch2, n=64, m=10)]
    lines = []
    for shape in shapes:
        B, n, m = shape["B"], shape["n"], shape["m"]
        x0_64 = amd.synthetic_x0_host(B, n, "std")
        x0_32 = x0_64.astype(np.float32)
        d64 = torch.from_numpy(x0_32.astype(np.float64)).to("cuda:0")   # the same starts: the float values, widened
        d32 = torch.from_numpy(x0_32).to("cuda:0")
        solvers = {
            "float32": (amd.BatchedLbfgs(m=m, stopping_progress=capi.default_stop(), context=ctx, arithmetic="exact",
                                         dtype=torch.float32), d32),
            "float64_exact_lds": (amd.BatchedLbfgs(m=m, stopping_progress=capi.default_stop(), context=ctx,
                                                   arithmetic="exact", history_placement=1), d64),
        }
        for solver, x0 in solvers.values():   # warm-up: code objects, staging, clocks
            run(solver, amd.Rosenbrock(), x0, amd, torch)
        per = {k: [] for k in solvers}
        for r in range(args.rounds):
            for key, (solver, x0) in solvers.items():
                ms, iters, prog, f = run(solver, amd.Rosenbrock(), x0, amd, torch)
                ll = solver.last_launch()
                line = dict(shape=shape["name"], B=B, n=n, m=m, precision=key, round=r, kernel_ms=ms,
                            solves_per_s=B / (ms * 1e-3), sum_num_iterations=iters,
                            kernel_ms_per_problem_iteration=ms / iters,
                            converged=int(np.isin(prog["status"], (3, 4)).sum()),
                            median_f=float(np.median(f.cpu().numpy())), lanes_per_problem=ll["lanes_per_problem"],
                            elems_per_lane=ll["elems_per_lane"], blocks=ll["blocks"], lds_bytes=ll["lds_bytes"])
                per[key].append(line)
                lines.append(line)
        med = {k: statistics.median(v["kernel_ms_per_problem_iteration"] for v in per[k]) for k in per}
        lines.append(dict(shape=shape["name"], summary=True, rounds=args.rounds,
                          median_kernel_ms={k: statistics.median(v["kernel_ms"] for v in per[k]) for k in per},
                          median_solves_per_s={k: statistics.median(v["solves_per_s"] for v in per[k]) for k in per},
                          median_kernel_ms_per_problem_iteration=med,
                          spread_kernel_ms={k: [min(v["kernel_ms"] for v in per[k]), max(v["kernel_ms"] for v in per[k])]
                                            for k in per},
                          float_over_double_per_problem_iteration=med["float32"] / med["float64_exact_lds"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
            if line.get("summary"):
                print(json.dumps(line))
    ctx.close()


if __name__ == "__main__":
    main()
