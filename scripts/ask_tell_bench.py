"""The ask/tell L-BFGS path next to the persistent exact kernel on the same batch (needs an MI355X).

65,536 x Rosenbrock-32, m = 6, parity stop (BASELINE.json configs[1]).  The callback of the ask/tell solve is the
library's own evaluation entry (BatchedLbfgs.evaluate), so both paths compute the same bits and the difference is the
price of reverse communication alone: one evaluation launch and one step launch per round, the history in HBM.
In one process, after a warm-up of each, `--repeats` times alternating:
  persistent   BatchedLbfgs(arithmetic="exact").minimize: kernel time from device events (last_kernel_ms) and the host
               clock around the call and a synchronise
  ask_tell     minimize_callable with check_every = 1 (the count is read back every round) and with check_every = 16:
               host clock around the whole loop, which ends in a synchronise
and once more by hand through LbfgsAskTell to record the problems still active after every round.
Prints a text report and writes it to --out.  No figure is asserted.
    python scripts/ask_tell_bench.py [--repeats 3] [--batch 65536] [--out profiles/ask_tell_rounds.txt]

--compact-every K[,K...] measures the LISTED mode instead: minimize_callable(compact_every=K) for every
K next to the uncompacted loop with check_every = 1 and 16 IN THE SAME RUN, alternating, after a warm-up of each (every
path must return the persistent kernel's bits: checked).  Beside the host-clock times it reports the rounds and the
deterministic figure the mode exists for: the ROWS the callback evaluated (the sum of `listed` over the rounds) against
batch x rounds.  That report goes to profiles/ask_tell_compact_rounds.txt unless --out says otherwise.
    python scripts/ask_tell_bench.py --compact-every 1,4,16,64"""
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--compact-every", default=None, help="comma-separated K: measure the listed mode (see above)")
    args = ap.parse_args()
    every = [int(k) for k in args.compact_every.split(",")] if args.compact_every else []
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ask_tell_compact_rounds.txt" if every else "ask_tell_rounds.txt")
    import torch
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    import cppnumericalsolvers_amd as amd

    B, n, m = args.batch, 32, 6
    ctx = amd.Context(0)
    solver = amd.BatchedLbfgs(m=m, stopping_progress=amd.parity_stop(), context=ctx, arithmetic="exact")
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

    def listed(k):
        rounds, seen = [0], [0]

        def fn(X, ids):
            rounds[0] += 1
            seen[0] += X.shape[0]
            return solver.evaluate(objective, X)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = solver.minimize_callable(fn, x0, compact_every=k)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3, rounds[0], seen[0]

    if every:
        compact_report(args, torch, B, n, m, every, persistent, ask_tell, listed)
        ctx.close()
        return

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

    # the problems still active after every round
    active = []
    with amd.LbfgsAskTell(solver, x0) as at:
        while True:
            count = at.tell(*solver.evaluate(objective, at.x))
            active.append(count)
            if count == 0:
                break
    prog = amd.progress_to_numpy(want[3])

    med = {k: statistics.median(v) for k, v in rows.items()}
    lines = []
    out = lines.append
    out("ask/tell L-BFGS next to the persistent exact kernel: %d x Rosenbrock-%d, m = %d, parity stop, one MI355X" % (B, n, m))
    out("callback: the library's evaluation entry (same bits on both paths: checked); %d repeats, medians [min, max]" % args.repeats)
    out("batch: sum of iterations %d, sum of evaluations %d, largest nfev of a problem %d"
        % (int(prog["num_iterations"].sum()), int(prog["nfev"].sum()), int(prog["nfev"].max())))
    for key, name in (("persistent_kernel", "persistent kernel (device events)"), ("persistent_wall", "persistent, host clock"),
                      (1, "ask/tell, check_every = 1, host clock"), (16, "ask/tell, check_every = 16, host clock")):
        out("  %-42s %10.3f ms  [%.3f, %.3f]" % (name, med[key], min(rows[key]), max(rows[key])))
    for k in (1, 16):
        out("  ask/tell check_every = %-2d: %d rounds, %.4f ms per round, %.1f x the persistent kernel, %.1f x its host-clock time"
            % (k, rounds_of[k], med[k] / rounds_of[k], med[k] / med["persistent_kernel"], med[k] / med["persistent_wall"]))
    out("problems still active after round r (of %d rounds):" % len(active))
    marks = sorted(set([1, 2, 3, 5, 10, 20, 30, 50, 75, 100, 150, 200, 300, 500, 750, 1000, 1500, 2000, 3000, 5000,
                        len(active)]))
    for r in marks:
        if r <= len(active):
            out("  r = %5d  active %7d  (%.2f %%)" % (r, active[r - 1], 100.0 * active[r - 1] / B))
    half = next(i + 1 for i, c in enumerate(active) if c <= B // 2)
    one_percent = next(i + 1 for i, c in enumerate(active) if c <= B // 100)
    out("  half of the batch has finished after %d rounds, 99 %% after %d, all after %d" % (half, one_percent, len(active)))
    out("  rounds x batch = %d problem-rounds, of which %d (%.1f %%) advanced an active problem"
        % (len(active) * B, B + sum(active[:-1]), 100.0 * (B + sum(active[:-1])) / (len(active) * B)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    ctx.close()


def compact_report(args, torch, B, n, m, every, persistent, ask_tell, listed):
    """the listed mode next to the uncompacted loop, in one run"""
    want, _, _ = persistent()          # warm-up of every path, and the bits
    for check in (1, 16):
        got, _, _ = ask_tell(check)
        for a, b in zip(got, want):
            assert torch.equal(a, b), "the uncompacted loop must return the persistent kernel's bits"
    for k in every:
        got, _, _, _ = listed(k)
        for a, b in zip(got, want):
            assert torch.equal(a, b), "the listed loop must return the persistent kernel's bits"
    wall = {("check", c): [] for c in (1, 16)}
    wall.update({("compact", k): [] for k in every})
    rounds_of, rows_of = {}, {}
    for _ in range(args.repeats):
        for c in (1, 16):
            _, ms, rounds_of[("check", c)] = ask_tell(c)
            wall[("check", c)].append(ms)
        for k in every:
            _, ms, rounds_of[("compact", k)], rows_of[k] = listed(k)
            wall[("compact", k)].append(ms)
    med = {key: statistics.median(v) for key, v in wall.items()}
    base = med[("check", 16)]
    spread = max((max(v) - min(v)) / statistics.median(v) for v in wall.values())
    lines = []
    out = lines.append
    out("ask/tell L-BFGS, listed mode next to the uncompacted loop: %d x Rosenbrock-%d, m = %d, parity stop, one MI355X" % (B, n, m))
    out("callback: the library's evaluation entry (every loop returns the persistent kernel's bits: checked); one run,")
    out("%d alternating repeats after a warm-up of each, host clock around the whole loop, medians [min, max]" % args.repeats)
    for c in (1, 16):
        key = ("check", c)
        out("  uncompacted, check_every = %-2d  %10.3f ms  [%.3f, %.3f]  %5d rounds  rows evaluated %11d (all of batch x rounds)"
            % (c, med[key], min(wall[key]), max(wall[key]), rounds_of[key], B * rounds_of[key]))
    for k in every:
        key = ("compact", k)
        out("  compact_every = %-3d            %10.3f ms  [%.3f, %.3f]  %5d rounds  rows evaluated %11d (%.1f %% of batch x rounds)  %.3f x check_every = 16"
            % (k, med[key], min(wall[key]), max(wall[key]), rounds_of[key], rows_of[k],
               100.0 * rows_of[k] / (B * rounds_of[key]), med[key] / base))
    out("largest (max - min) / median of a row above: %.1f %%" % (100.0 * spread))
    faster = [k for k in every if med[("compact", k)] < base * (1.0 - spread)]
    slower = [k for k in every if k not in faster]
    out("faster than the uncompacted check_every = 16 loop beyond that spread: compact_every in %s; not faster: %s"
        % (faster or "none", slower or "none"))
    out("(the callback here is the cheapest there is; the rows evaluated are what an expensive callback pays for)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
