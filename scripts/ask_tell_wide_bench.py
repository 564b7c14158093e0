"""The ask/tell L-BFGS loop above n = 256 next to the persistent wide kernel (needs an MI355X).

Rosenbrock, m = 10, an iteration limit of 100 under the parity stop, at 2048 x 1024, 2048 x 4096 and 256 x 16384.  The
callback of every ask/tell solve is the library's own evaluation entry (BatchedLbfgs.evaluate above n = 256), so the
loop computes the bits of the persistent kernel (checked) and the difference is the price of reverse communication.
Per shape, in one process, after a warm-up of each, `--repeats` times alternating:
  persistent     BatchedLbfgs.minimize (lbfgs_wide_kernel): device events and the host clock
  ask/tell       minimize_callable, check_every = 1 and 16: host clock around the whole loop, which ends in a synchronise
  ask/tell, direction in memory   the same with MI355_WIDE_LDS_MAX_N=0 around the loop (n <= 4096 only)
and once more by hand through LbfgsAskTell, reading the device events of every step call (mi355_lbfgs_last_kernel_ms;
this run waits for every call, so its host clock is not reported), with the direction in LDS and in memory.
Bytes a step MUST move (a floor: every vector a part reads or writes counted once per part, 8 n bytes each, caches
ignored), summed over the solve from the progress records — E = nfev - 1 trial evaluations, I iterations, K = sum_k
history pairs used, per problem:
  evaluated trial    2 E        the caller's gradient and d
  next trial         3 (E - I)  d, x in, x_eval out (a search's last evaluation asks for no further trial)
  update             12 I       next and current x, g in twice (sums, then the pair), s, y, x, g out
  recursion          (4 K + 2 I) the ring vectors and g; with the direction in memory (4 K + I) more for d itself
  first trial        3 I        x in, d and x_eval out (4 I with the direction in memory: d in)
Prints a text report and writes it to --out.  No figure is asserted.
    python scripts/ask_tell_wide_bench.py [--repeats 3] [--out profiles/ask_tell_wide_rounds.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LDS_ENV = "MI355_WIDE_LDS_MAX_N"
SHAPES = ((2048, 1024), (2048, 4096), (256, 16384))


def model_bytes(p, n, in_memory):
    E = p["nfev"].astype(np.float64) - 1.0
    I = p["num_iterations"].astype(np.float64)
    K = p["sum_k"].astype(np.float64)
    vectors = 2 * E + 3 * np.maximum(E - I, 0) + 12 * I + 4 * K + 2 * I + 3 * I
    if in_memory:
        vectors = vectors + 4 * K + I + I
    return float(vectors.sum()) * 8.0 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ask_tell_wide_rounds.txt"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    import cppnumericalsolvers_amd as amd

    m = 10
    stop = amd.parity_stop()
    stop.num_iterations = 100
    ctx = amd.Context(0)
    solver = amd.BatchedLbfgs(m=m, stopping_progress=stop, context=ctx, arithmetic="exact")
    objective = amd.Rosenbrock()
    lines = []
    out = lines.append
    out("ask/tell L-BFGS above n = 256 next to the persistent wide kernel: Rosenbrock, m = %d, parity stop with an iteration "
        "limit of 100, one MI355X" % m)
    out("callback: the library's evaluation entry (ask/tell loop == persistent kernel, bit for bit: checked); %d repeats, "
        "medians [min, max]" % args.repeats)

    def persistent(x0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = solver.minimize(objective, x0)
        torch.cuda.synchronize()
        return res, (time.perf_counter() - t0) * 1e3, solver.last_kernel_ms()

    def ask_tell(x0, check_every, in_memory=False):
        rounds = [0]

        def fn(X):
            rounds[0] += 1
            return solver.evaluate(objective, X)
        if in_memory:
            os.environ[LDS_ENV] = "0"
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = solver.minimize_callable(fn, x0, check_every=check_every)
            torch.cuda.synchronize()
            return res, (time.perf_counter() - t0) * 1e3, rounds[0]
        finally:
            os.environ.pop(LDS_ENV, None)

    def by_hand(x0, in_memory):
        """device-clock ms of every step call and of every evaluation call"""
        steps, evals = [], []
        if in_memory:
            os.environ[LDS_ENV] = "0"
        try:
            with amd.LbfgsAskTell(solver, x0) as at:
                while True:
                    f, g = solver.evaluate(objective, at.x)
                    evals.append(solver.last_kernel_ms())
                    count = at.tell(f, g)
                    steps.append(solver.last_kernel_ms())
                    if count == 0:
                        break
                lds = solver.last_launch()["lds_bytes"]
        finally:
            os.environ.pop(LDS_ENV, None)
        return steps, evals, lds

    for B, n in SHAPES:
        x0 = torch.from_numpy(amd.synthetic_x0_host(B, n, "std")).to("cuda:0")
        forms = [False] + ([True] if n <= 4096 else [])
        loops = [(k, mem) for mem in forms for k in (1, 16)]
        want, _, _ = persistent(x0)            # warm-up of every path: code objects, allocator, clocks
        for key in loops:
            got, _, _ = ask_tell(x0, *key)
            for a, b in zip(got, want):
                assert torch.equal(a, b), "the ask/tell loop must return the bits of the persistent kernel"
        rows = {"persistent_wall": [], "persistent_kernel": [], **{key: [] for key in loops}}
        rounds_of = {}
        for _ in range(args.repeats):
            _, wall, kernel = persistent(x0)
            rows["persistent_wall"].append(wall)
            rows["persistent_kernel"].append(kernel)
            for key in loops:
                _, wall, rounds = ask_tell(x0, *key)
                rows[key].append(wall)
                rounds_of[key] = rounds
        p = amd.progress_to_numpy(want[3])
        med = {k: statistics.median(v) for k, v in rows.items()}
        out("")
        out("%d x %d: sum of iterations %d, sum of evaluations %d, largest nfev of a problem %d, sum_k %d; statuses %s; "
            "state of the handle %.1f MB"
            % (B, n, int(p["num_iterations"].sum()), int(p["nfev"].sum()), int(p["nfev"].max()), int(p["sum_k"].sum()),
               dict(zip(*[v.tolist() for v in np.unique(p["status"], return_counts=True)])),
               B * ((3 + 2 * m) * (n + n % 2) + n) * 8 / 1e6))
        names = [("persistent_kernel", "persistent kernel (device events)"), ("persistent_wall", "persistent, host clock")]
        names += [((k, mem), "ask/tell, check_every = %d, direction in %s, host clock" % (k, "memory" if mem else
                                                                                        ("LDS" if n <= 4096 else "memory")))
                  for k, mem in loops]
        for key, name in names:
            out("  %-62s %10.3f ms  [%.3f, %.3f]" % (name, med[key], min(rows[key]), max(rows[key])))
        for key in loops:
            ratios = sorted(a / b for a, b in zip(rows[key], rows["persistent_kernel"]))
            out("  check_every = %-2d%s: %d rounds, %.4f ms per round; loop / persistent kernel = %.2f [%.2f, %.2f]"
                % (key[0], " (direction in memory)" if key[1] else "", rounds_of[key], med[key] / rounds_of[key],
                   statistics.median(ratios), ratios[0], ratios[-1]))
        for mem in forms:
            steps, evals, lds = by_hand(x0, mem)
            in_memory = mem or n > 4096
            assert (lds == 0) == in_memory
            total_s, total_e = sum(steps), sum(evals)
            floor = model_bytes(p, n, in_memory)
            out("  by hand, direction in %s (dynamic LDS %d B): %d step calls, device clock %.1f us per call (median %.1f, "
                "max %.1f), %.3f ms in all; evaluation calls %.1f us per call, %.3f ms in all"
                % ("memory" if in_memory else "LDS", lds, len(steps), 1e3 * total_s / len(steps),
                   1e3 * statistics.median(steps), 1e3 * max(steps), total_s, 1e3 * total_e / len(evals), total_e))
            out("    bytes the steps must move (floor, see the script): %.3f GB = %.2f MB per call; / device time of the steps = "
                "%.0f GB/s" % (floor / 1e9, floor / 1e6 / len(steps), floor / 1e9 / (total_s / 1e3)))
            out("    steps + evaluations on the device clock / persistent kernel = %.2f"
                % ((total_s + total_e) / med["persistent_kernel"]))
        del x0
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
