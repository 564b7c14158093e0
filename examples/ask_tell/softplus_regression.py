"""Your own objective without a build: B small regressions with a softplus link, one data set per problem.

    f_b(w) = sum_i softplus(a_bi . w) - y_bi (a_bi . w) + 1/2 lambda ||w||^2        (logistic regression, labels in {0, 1})

The objective is plain torch code on the solver's [B, n] tensor of trial points and returns the B values only: the
gradient comes from autograd.  Nothing is compiled: BatchedLbfgs.minimize_callable keeps the state of every problem on
the device (history, line search, stopping tests) and asks for one batched evaluation per round.  Needs an MI355X.
    python examples/ask_tell/softplus_regression.py [--problems 4096] [--rows 64] [--features 10]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--features", type=int, default=10)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi

    B, rows, n, lam = args.problems, args.rows, args.features, 0.1
    gen = torch.Generator().manual_seed(20261019)
    A = torch.randn(B, rows, n, generator=gen, dtype=torch.float64).to("cuda:0")       # per-problem data
    w_true = torch.randn(B, n, generator=gen, dtype=torch.float64).to("cuda:0")
    y = (torch.rand(B, rows, generator=gen, dtype=torch.float64).to("cuda:0") <
         torch.sigmoid(torch.einsum("brn,bn->br", A, w_true))).to(torch.float64)

    def value(W):                                                                       # [B, n] -> [B]
        z = torch.einsum("brn,bn->br", A, W)
        return (torch.nn.functional.softplus(z) - y * z).sum(dim=1) + 0.5 * lam * (W * W).sum(dim=1)

    stop = capi.default_stop()
    stop.gradient_norm, stop.past = 1e-8, 0
    solver = amd.BatchedLbfgs(m=10, stopping_progress=stop, arithmetic="exact")
    w, f, g, progress = solver.minimize_callable(value, torch.zeros(B, n, dtype=torch.float64, device="cuda:0"))
    torch.cuda.synchronize()
    p = amd.progress_to_numpy(progress)
    print("%d problems: statuses %s, iterations median %d max %d, evaluations max %d, max ||g||inf %.3g"
          % (B, {int(k): int(v) for k, v in zip(*np.unique(p["status"], return_counts=True))}, int(np.median(p["num_iterations"])),
             int(p["num_iterations"].max()), int(p["nfev"].max()), float(g.abs().max())))


if __name__ == "__main__":
    main()
