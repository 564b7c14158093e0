"""The ask/tell L-BFGS-B path next to the persistent reference-order kernel on the same batch (needs an MI355X).

65,536 x Rosenbrock-32 in the box [-1.5, 0.8], m = 5, the default Lbfgsb stop.  The callback of the ask/tell solve is the
library's own evaluation entry (BatchedLbfgsb.evaluate), so both paths compute the same bits and the difference is the
price of reverse communication alone: one evaluation launch and one step launch per round, the state in HBM.
In one process, after a warm-up of each, `--repeats` times alternating:
  persistent   BatchedLbfgsb(arithmetic="exact").minimize: kernel time from device events and the host clock
  ask_tell     minimize_callable with check_every = 1 and with check_every = 16: host clock around the whole loop
and once more by hand through LbfgsbAskTell to record the problems still active after every round and the ask counters.
Prints a text report and writes it to --out.  No figure is asserted.
    python scripts/ask_tell_box_bench.py [--repeats 3] [--batch 65536] [--out profiles/ask_tell_box_rounds.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ask_tell_box_rounds.txt"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    import cppnumericalsolvers_amd as amd

    B, n, m = args.batch, 32, 5
    ctx = amd.Context(0)
    solver = amd.BatchedLbfgsb(m=m, context=ctx, arithmetic="exact")
    solver.SetBounds(np.full(n, -1.5), np.full(n, 0.8))
    objective = amd.Rosenbrock()
    x0 = torch.from_numpy(amd.synthetic_x0_host(B, n, "std")).to("cuda:0")

    def persistent():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = solver.minimize(objective, x0)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return out, wall, solver.last_kernel_ms()

    def ask_tell(check_every):
        rounds = [0]

        def fn(X):
            rounds[0] += 1
            return solver.evaluate(objective, X)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = solver.minimize_callable(fn, x0, check_every=check_every)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3, rounds[0]

    want, _, _ = persistent()          # warm-up of every path: code objects, allocator, clocks
    for k in (1, 16):
        got, _, _ = ask_tell(k)
        for a, b in zip(got, want):
            assert torch.equal(a, b), "the two paths must return the same bits"
    rows = {"persistent_wall": [], "persistent_kernel": [], 1: [], 16: []}
    rounds_of = {}
    for _ in range(args.repeats):
        _, wall, kernel = persistent()
        rows["persistent_wall"].append(wall)
        rows["persistent_kernel"].append(kernel)
        for k in (1, 16):
            _, wall, rounds = ask_tell(k)
            rows[k].append(wall)
            rounds_of[k] = rounds

    # the problems still active after every round, and what was asked for
    active = []
    with amd.LbfgsbAskTell(solver, x0) as at:
        while True:
            count = at.tell(*solver.evaluate(objective, at.x))
            active.append(count)
            if count == 0:
                break
        asks = at.asks
    prog = amd.progress_to_numpy(want[3])

    med = {k: statistics.median(v) for k, v in rows.items()}
    lines = []
    out = lines.append
    out("ask/tell L-BFGS-B next to the persistent reference-order kernel: %d x Rosenbrock-%d in [-1.5, 0.8], m = %d, "
        "default Lbfgsb stop, one MI355X" % (B, n, m))
    out("callback: the library's evaluation entry (same bits on both paths: checked); %d repeats, medians [min, max]" % args.repeats)
    out("batch: sum of iterations %d, sum of evaluations %d, largest nfev of a problem %d"
        % (int(prog["num_iterations"].sum()), int(prog["nfev"].sum()), int(prog["nfev"].max())))
    for key, name in (("persistent_kernel", "persistent kernel (device events)"), ("persistent_wall", "persistent, host clock"),
                      (1, "ask/tell, check_every = 1, host clock"), (16, "ask/tell, check_every = 16, host clock")):
        out("  %-42s %10.3f ms  [%.3f, %.3f]" % (name, med[key], min(rows[key]), max(rows[key])))
    for k in (1, 16):
        out("  ask/tell check_every = %-2d: %d rounds, %.4f ms per round, %.1f x the persistent kernel, %.1f x its host-clock time"
            % (k, rounds_of[k], med[k] / rounds_of[k], med[k] / med["persistent_kernel"], med[k] / med["persistent_wall"]))
    out("asks: " + ", ".join("%s %d" % kv for kv in asks.items()) + "  (sum %d)" % sum(asks.values()))
    out("problems still active after round r (of %d rounds):" % len(active))
    marks = sorted(set([1, 2, 3, 5, 10, 20, 30, 50, 75, 100, 150, 200, 300, 500, 750, 1000, 1500, 2000, 3000, 5000,
                        len(active)]))
    for r in marks:
        if r <= len(active):
            out("  r = %5d  active %7d  (%.2f %%)" % (r, active[r - 1], 100.0 * active[r - 1] / B))
    out("  rounds x batch = %d problem-rounds, of which %d (%.1f %%) advanced an active problem"
        % (len(active) * B, B + sum(active[:-1]), 100.0 * (B + sum(active[:-1])) / (len(active) * B)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
