#!/usr/bin/env python
"""GradientDescent and ConjugatedGradientDescent throughput on one MI355X (csrc/first_order_kernel.hpp), with BatchedLbfgs
on the same batch for scale: Rosenbrock-8 / -32 / -64 / -256 from the bench's synthetic starts
(amd.synthetic_x0_host), ONE stop for every row: the default stopping preset with num_iterations capped at 200 (first-order
methods need thousands of iterations on Rosenbrock; the cap makes the rows comparable and short).  Per shape: kernel ms
(the context's events) as the median of --reps runs after a warm-up, with min and max, solves/s, and the mean / max of
iterations, nfev and trial points per solve.  ConjugatedGradientDescent is measured in both trial variants: value-only
trials with one final eval (the default) and eval on every trial (a context created under MI355_DEBUG_CG_EVAL_TRIALS=1).
One JSON object per line (JSON lines) on stdout; --out also writes them to a file.

    python scripts/first_order_bench.py --out profiles/first_order_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ITERATION_CAP = 200
KNOB = "MI355_DEBUG_CG_EVAL_TRIALS"


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    os.environ.pop(KNOB, None)
    plain = amd.Context(0)
    os.environ[KNOB] = "1"
    eval_trials = amd.Context(0)
    os.environ.pop(KNOB, None)

    def stop():
        s = capi.default_stop()
        s.num_iterations = ITERATION_CAP
        return s
    rows = []
    for B, n in ((65536, 8), (65536, 32), (16384, 64), (4096, 256)):
        x0 = torch.from_numpy(amd.synthetic_x0_host(B, n, "std")).to("cuda:0")
        runs = [("gradient_descent", amd.BatchedGradientDescent(stopping_progress=stop(), context=plain)),
                ("conjugated_gradient_descent, value trials",
                 amd.BatchedConjugatedGradientDescent(stopping_progress=stop(), context=plain)),
                ("conjugated_gradient_descent, eval trials",
                 amd.BatchedConjugatedGradientDescent(stopping_progress=stop(), context=eval_trials)),
                ("lbfgs", amd.BatchedLbfgs(stopping_progress=stop(), context=plain))]
        for name, solver in runs:
            run(solver, amd.Rosenbrock(), x0, 1)   # warm-up
            ms, p = run(solver, amd.Rosenbrock(), x0, args.reps)
            med = float(np.median(ms))
            ll = solver.last_launch()
            row = dict(solver=name, B=B, n=n, stop="default, num_iterations=%d" % ITERATION_CAP,
                       lanes_per_problem=ll["lanes_per_problem"], elems_per_lane=ll["elems_per_lane"],
                       blocks=ll["blocks"], kernel_ms=round(med, 3), kernel_ms_min=round(min(ms), 3),
                       kernel_ms_max=round(max(ms), 3), reps=args.reps, solves_per_s=round(B / (med * 1e-3)),
                       iterations_mean=round(float(p["num_iterations"].mean()), 2),
                       iterations_max=int(p["num_iterations"].max()), nfev_mean=round(float(p["nfev"].mean()), 2),
                       nfev_max=int(p["nfev"].max()),
                       status_counts={int(s): int(c) for s, c in zip(*np.unique(p["status"], return_counts=True))})
            if name != "lbfgs":
                row["trials_mean"] = round(float(p["sum_k"].mean()), 2)
                row["trials_max"] = int(p["sum_k"].max())
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
