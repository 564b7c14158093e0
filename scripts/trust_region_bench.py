#!/usr/bin/env python
"""TrustRegionNewton throughput on one MI355X (csrc/trust_region_kernel.hpp), with BatchedLbfgs on the same batch:
65,536 x Rosenbrock-32 and 16,384 x Rosenbrock-64 from the bench's synthetic starts (amd.synthetic_x0_host), default
stopping preset and config.  Per shape and lane mapping: kernel ms (median, min and max of --reps), solves/s, and the mean / max of
iterations, nfev and CG iterations.  The mapping sweep covers every padded width: n = 8, 16, 32 at their own width and
at the next ones, n = 64 at 64 (65,536 problems at n <= 32).  One JSON object per line (JSON lines) on stdout; --out also
writes them to a file.

    python scripts/trust_region_bench.py --out profiles/trust_region_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(solver, obj, x0, reps):
    import torch
    import cppnumericalsolvers_amd as amd
    ms = []
    for _ in range(reps):
        x, f, g, p = solver.minimize(obj, x0)
        torch.cuda.synchronize()
        ms.append(solver.last_kernel_ms())
    return ms, amd.progress_to_numpy(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import cppnumericalsolvers_amd as amd
    rows = []
    for B, n in ((65536, 8), (65536, 16), (65536, 32), (16384, 64)):
        x0 = torch.from_numpy(amd.synthetic_x0_host(B, n, "std")).to("cuda:0")
        runs = [("trust_region", lanes, amd.BatchedTrustRegionNewton(lanes_per_problem=lanes)) for lanes in
                (8, 16, 32, 64) if n <= lanes <= max(2 * n, 64 if n >= 32 else 2 * n)]
        if n >= 32:
            runs.append(("lbfgs", 0, amd.BatchedLbfgs()))
        for name, lanes, solver in runs:
            run(solver, amd.Rosenbrock(), x0, 1)   # warm-up
            all_ms, p = run(solver, amd.Rosenbrock(), x0, args.reps)
            ms = float(np.median(all_ms))
            row = dict(solver=name, B=B, n=n, lanes_per_problem=lanes or "auto", kernel_ms=round(ms, 3),
                       kernel_ms_min=round(min(all_ms), 3), kernel_ms_max=round(max(all_ms), 3), reps=args.reps,
                       solves_per_s=round(B / (ms * 1e-3)), iterations_mean=round(float(p["num_iterations"].mean()), 2),
                       iterations_max=int(p["num_iterations"].max()), nfev_mean=round(float(p["nfev"].mean()), 2),
                       status_counts={int(s): int(c) for s, c in zip(*np.unique(p["status"], return_counts=True))})
            if name == "trust_region":
                row["cg_iterations_mean"] = round(float(p["sum_k"].mean()), 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
