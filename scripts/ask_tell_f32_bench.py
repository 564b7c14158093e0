"""The float ask/tell L-BFGS loop next to the persistent float kernel and next to the fp64 ask/tell loop (needs an MI355X).

65,536 x Rosenbrock-32, m = 6, the reference's default stop, the protocol of scripts/ask_tell_bench.py.  The callback of
every ask/tell solve is the library's own evaluation entry of its precision (BatchedLbfgs.evaluate), so the float loop
computes the bits of the persistent float kernel (checked) and the difference is the price of reverse communication.
The fp64 loop runs from the same starts (the float32 starts widened).  In one process, after a warm-up of each,
`--repeats` times alternating:
  persistent f32   BatchedLbfgs(dtype=float32, arithmetic="exact").minimize: device events and the host clock
  ask/tell f32     minimize_callable, check_every = 1 and 16: host clock around the whole loop, which ends in a synchronise
  ask/tell f64     the same on a float64 solver
and once more by hand through LbfgsAskTell, in each precision, to count the problems still active after every round.
Prints a text report and writes it to --out.  No figure is asserted.
    python scripts/ask_tell_f32_bench.py [--repeats 3] [--batch 65536] [--out profiles/ask_tell_f32_rounds.txt]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ask_tell_f32_rounds.txt"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi

    B, n, m = args.batch, 32, 6
    ctx = amd.Context(0)
    solvers = {"f32": amd.BatchedLbfgs(m=m, stopping_progress=capi.default_stop(), context=ctx, arithmetic="exact",
                                       dtype=torch.float32),
               "f64": amd.BatchedLbfgs(m=m, stopping_progress=capi.default_stop(), context=ctx, arithmetic="exact")}
    objective = amd.Rosenbrock()
    x0_host = amd.synthetic_x0_host(B, n, "std").astype(np.float32)
    x0 = {"f32": torch.from_numpy(x0_host).to("cuda:0"), "f64": torch.from_numpy(x0_host.astype(np.float64)).to("cuda:0")}

    def persistent():
        solver = solvers["f32"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = solver.minimize(objective, x0["f32"])
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return out, wall, solver.last_kernel_ms()

    def ask_tell(which, check_every):
        solver = solvers[which]
        rounds = [0]

        def fn(X):
            rounds[0] += 1
            return solver.evaluate(objective, X)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = solver.minimize_callable(fn, x0[which], check_every=check_every)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3, rounds[0]

    loops = [(which, k) for which in ("f32", "f64") for k in (1, 16)]
    want, _, _ = persistent()          # warm-up of every path: code objects, allocator, clocks
    results = {}
    for which, k in loops:
        got, _, _ = ask_tell(which, k)
        results[which] = got
        if which == "f32":
            for a, b in zip(got, want):
                assert torch.equal(a, b), "the float ask/tell loop must return the bits of the persistent float kernel"
    rows = {"persistent_wall": [], "persistent_kernel": [], **{key: [] for key in loops}}
    rounds_of = {}
    for _ in range(args.repeats):
        _, wall, kernel = persistent()
        rows["persistent_wall"].append(wall)
        rows["persistent_kernel"].append(kernel)
        for key in loops:
            _, wall, rounds = ask_tell(*key)
            rows[key].append(wall)
            rounds_of[key] = rounds

    # the problems still active after every round
    active = {}
    for which in ("f32", "f64"):
        solver, counts = solvers[which], []
        with amd.LbfgsAskTell(solver, x0[which]) as at:
            while True:
                count = at.tell(*solver.evaluate(objective, at.x))
                counts.append(count)
                if count == 0:
                    break
        active[which] = counts
    prog = {which: amd.progress_to_numpy(results[which][3]) for which in ("f32", "f64")}

    med = {k: statistics.median(v) for k, v in rows.items()}
    lines = []
    out = lines.append
    out("float ask/tell L-BFGS next to the persistent float kernel and the fp64 ask/tell loop: %d x Rosenbrock-%d, m = %d, "
        "the reference's default stop, one MI355X" % (B, n, m))
    out("callback: the library's evaluation entry of each precision (float loop == persistent float kernel, bit for bit: "
        "checked); %d repeats, medians [min, max]" % args.repeats)
    for which in ("f32", "f64"):
        p = prog[which]
        out("batch, %s: sum of iterations %d, sum of evaluations %d, largest nfev of a problem %d; statuses %s"
            % (which, int(p["num_iterations"].sum()), int(p["nfev"].sum()), int(p["nfev"].max()),
               dict(zip(*[v.tolist() for v in np.unique(p["status"], return_counts=True)]))))
    names = [("persistent_kernel", "persistent f32 kernel (device events)"), ("persistent_wall", "persistent f32, host clock")]
    names += [((which, k), "ask/tell %s, check_every = %d, host clock" % (which, k)) for which, k in loops]
    for key, name in names:
        out("  %-44s %10.3f ms  [%.3f, %.3f]" % (name, med[key], min(rows[key]), max(rows[key])))
    for which, k in loops:
        key = (which, k)
        out("  ask/tell %s check_every = %-2d: %d rounds, %.4f ms per round [%.4f, %.4f]"
            % (which, k, rounds_of[key], med[key] / rounds_of[key], min(rows[key]) / rounds_of[key],
               max(rows[key]) / rounds_of[key]))
    for k in (1, 16):
        ratios_p = sorted(a / b for a, b in zip(rows[("f32", k)], rows["persistent_kernel"]))
        ratios_d = sorted(a / b for a, b in zip(rows[("f32", k)], rows[("f64", k)]))
        per_round = sorted((a / rounds_of[("f32", k)]) / (b / rounds_of[("f64", k)])
                           for a, b in zip(rows[("f32", k)], rows[("f64", k)]))
        out("  check_every = %-2d: f32 loop / persistent f32 kernel = %.2f [%.2f, %.2f]; f32 loop / f64 loop = %.3f "
            "[%.3f, %.3f] in total, %.3f [%.3f, %.3f] per round"
            % (k, statistics.median(ratios_p), ratios_p[0], ratios_p[-1], statistics.median(ratios_d), ratios_d[0],
               ratios_d[-1], statistics.median(per_round), per_round[0], per_round[-1]))
    marks = [1, 2, 3, 5, 10, 20, 30, 50, 75, 100, 150, 200, 300, 500, 750, 1000, 1500, 2000, 3000, 5000]
    for which in ("f32", "f64"):
        counts = active[which]
        out("%s: problems still active after round r (of %d rounds):" % (which, len(counts)))
        for r in sorted(set(marks + [len(counts)])):
            if r <= len(counts):
                out("  r = %5d  active %7d  (%.2f %%)" % (r, counts[r - 1], 100.0 * counts[r - 1] / B))
        half = next(i + 1 for i, c in enumerate(counts) if c <= B // 2)
        one_percent = next(i + 1 for i, c in enumerate(counts) if c <= B // 100)
        out("  half of the batch has finished after %d rounds, 99 %% after %d, all after %d" % (half, one_percent, len(counts)))
        out("  rounds x batch = %d problem-rounds, of which %d (%.1f %%) advanced an active problem"
            % (len(counts) * B, B + sum(counts[:-1]), 100.0 * (B + sum(counts[:-1])) / (len(counts) * B)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
