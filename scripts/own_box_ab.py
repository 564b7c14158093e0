#!/usr/bin/env python3
"""A/B of the per-problem-bounds entry against the shared-box entry on configs[4]'s shape (262,144 x Rosenbrock-32 in
[-1.5, 0.8]^32, m = 5, the bench's tight stopping), relaxed and exact arithmetic, on one GPU in one process:
  A/A   the shared entry against itself            -> the run-to-run spread
  A/B   the shared entry against the new entry with 262,144 identical rows (the same box in every row)
alternating the two sides, `last_kernel_ms` of every launch, the median of ROUNDS alternations after one warm-up each.
The results of the two sides are compared bit for bit.  Then the same with every solve cut off after 5 iterations: what
the new entry costs per FETCHED problem stays, what it costs per iteration shrinks with the solve.   python scripts/own_box_ab.py > profiles/own_box_ab.txt"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import cppnumericalsolvers_amd as amd  # noqa: E402

ROUNDS = 7
B, n, m = 262144, 32, 5


def tight_stop(num_iterations):
    s = amd.capi.default_stop("lbfgsb")
    s.num_iterations, s.x_delta, s.x_delta_violations = num_iterations, 1e-11, 1
    s.f_delta, s.f_delta_relative, s.gradient_norm, s.past = 0.0, 0, 1e-8, 0
    return s


def main():
    ctx = amd.Context(0)
    x0 = torch.from_numpy(amd.synthetic_x0_host(B, n, "u2")).cuda()
    lo, hi = np.full(n, -1.5), np.full(n, 0.8)
    rows_lo = torch.from_numpy(np.tile(lo, (B, 1))).cuda()
    rows_hi = torch.from_numpy(np.tile(hi, (B, 1))).cuda()
    print("Lbfgsb<F, %d>, %d x Rosenbrock-%d in [-1.5, 0.8]^%d, tight stopping; %s; kernel ms = last_kernel_ms, median of %d "
          "alternations" % (m, B, n, n, torch.cuda.get_device_name(0), ROUNDS))
    for arithmetic, limit in (("fma", 10000), ("exact", 10000), ("fma", 5), ("exact", 5)):
        def side(own):
            s = amd.BatchedLbfgsb(m=m, stopping_progress=tight_stop(limit), context=ctx, arithmetic=arithmetic)
            if own:
                s.SetBoundsPerProblem(rows_lo, rows_hi)
            else:
                s.SetBounds(lo, hi)
            return s
        for label, a, b in (("A/A shared vs shared", side(False), side(False)), ("A/B shared vs own box", side(False), side(True))):
            ms = {0: [], 1: []}
            out = {}
            for r in range(ROUNDS + 1):
                for i, s in enumerate((a, b)):
                    out[i] = s.minimize(amd.Rosenbrock(), x0)
                    torch.cuda.synchronize()
                    if r > 0:
                        ms[i].append(s.last_kernel_ms())
            same = all(torch.equal(u, v) for u, v in zip(out[0], out[1]))
            ma, mb = float(np.median(ms[0])), float(np.median(ms[1]))
            ll = b.last_launch()
            print("%-5s %5d iterations at most  %-22s first %8.3f ms [%7.3f .. %7.3f]  second %8.3f ms [%7.3f .. %7.3f]  second/first %.4f  same bits: %s  "
                  "(%d x %d, %d workgroups, %s)" % (arithmetic, limit, label, ma, min(ms[0]), max(ms[0]), mb, min(ms[1]), max(ms[1]),
                                                    mb / ma, same, ll["lanes_per_problem"], ll["elems_per_lane"], ll["blocks"],
                                                    b.last_arithmetic()))


if __name__ == "__main__":
    main()
