#!/usr/bin/env python
"""NelderMead throughput on one MI355X (csrc/nelder_mead_kernel.hpp): 65,536 x Rosenbrock-8 / -32 / -64 from the bench's
synthetic starts (amd.synthetic_x0_host), value mode, the solver's own stopping preset (conservative, five x_delta
strikes) and default coefficients, each n at its padded width.  Per shape: kernel ms (median of --reps after one
warm-up), solves/s, ms per step (kernel ms / the longest solve's steps: the kernel is done when its slowest segment is)
and the mean / max of iterations and nfev.  One JSON object per line on stdout; --out also writes them to a file.

    python scripts/nelder_mead_bench.py --out profiles/nelder_mead_bench.jsonl

--reference-lib PATH adds, beside each device row, the reference's own header on the host threads for the same batch:
PATH is the harness library tests/nm_lib.build_reference() compiles where the reference tree exists (it is not part of
the repository); the batch is split over --threads processes' worth of rows with a thread pool (ctypes releases the GIL).
--device none skips the device rows (a machine without a GPU that has the reference tree)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((65536, 8), (65536, 32), (65536, 64))


def summary(p):
    return dict(iterations_mean=round(float(p["num_iterations"].mean()), 2), iterations_max=int(p["num_iterations"].max()),
                nfev_mean=round(float(p["nfev"].mean()), 2),
                status_counts={int(s): int(c) for s, c in zip(*np.unique(p["status"], return_counts=True))})


def device_row(B, n, reps):
    import torch
    import cppnumericalsolvers_amd as amd
    x0 = torch.from_numpy(amd.synthetic_x0_host(B, n, "std")).to("cuda:0")
    solver = amd.BatchedNelderMead()
    ms = []
    for rep in range(reps + 1):   # the first is the warm-up
        x, f, g, p = solver.minimize(amd.Rosenbrock(), x0)
        torch.cuda.synchronize()
        if rep:
            ms.append(solver.last_kernel_ms())
    p = amd.progress_to_numpy(p)
    med = float(np.median(ms))
    return dict(solver="nelder_mead", where="device", B=B, n=n, mode="value",
                lanes_per_problem=solver.last_launch()["lanes_per_problem"], reps=reps, kernel_ms=round(med, 3),
                kernel_ms_min=round(min(ms), 3), kernel_ms_max=round(max(ms), 3), solves_per_s=round(B / (med * 1e-3)),
                ms_per_step=round(med / max(int(p["num_iterations"].max()), 1), 5), **summary(p))


def reference_row(lib, B, n, threads):
    import cppnumericalsolvers_amd as amd
    import nm_lib as T
    ref = T.reference_solver(lib)
    x0 = amd.synthetic_x0_host(B, n, "std")
    chunks = np.array_split(np.arange(B), threads * 4)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda idx: ref(T.ROSENBROCK, x0[idx])[3], chunks))
    wall = time.perf_counter() - t0
    p = np.concatenate(parts)
    return dict(solver="nelder_mead", where="reference header, host threads", B=B, n=n, mode="value", threads=threads,
                reps=1, wall_ms=round(wall * 1e3, 1), solves_per_s=round(B / wall), **summary(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda", choices=("cuda", "none"))
    ap.add_argument("--reference-lib", default=None)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    rows = []
    for B, n in SHAPES:
        if args.device == "cuda":
            rows.append(device_row(B, n, args.reps))
            print(json.dumps(rows[-1]), flush=True)
        if args.reference_lib:
            rows.append(reference_row(args.reference_lib, B, n, args.threads))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "a" if args.device == "none" else "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
