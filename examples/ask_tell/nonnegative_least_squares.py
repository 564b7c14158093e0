"""Bounds on the parameters of your own objective, without a build: B small non-negative least-squares problems.

    minimise  f_b(w) = 1/2 ||A_b w - y_b||^2      subject to  0 <= w <= 10

The objective is plain torch code on the solver's [B, n] tensor of points and returns the B values only: the gradient
comes from autograd.  Nothing is compiled: BatchedLbfgsb.minimize_callable keeps the state of every problem on the device
(the L-BFGS-B history and its compact representation, the line search, the stopping tests) and asks for one batched
evaluation per round.  The printed check is the KKT residual of the box: the projected gradient.  Needs an MI355X.
    python examples/ask_tell/nonnegative_least_squares.py [--problems 4096] [--rows 40] [--features 12]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=40)
    ap.add_argument("--features", type=int, default=12)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi

    B, rows, n = args.problems, args.rows, args.features
    gen = torch.Generator().manual_seed(20261019)
    A = torch.randn(B, rows, n, generator=gen, dtype=torch.float64).to("cuda:0")        # per-problem data
    w_true = torch.randn(B, n, generator=gen, dtype=torch.float64).clamp_min(0.0).to("cuda:0")   # half the weights are 0
    y = torch.einsum("brn,bn->br", A, w_true) + 0.05 * torch.randn(B, rows, generator=gen, dtype=torch.float64).to("cuda:0")

    def value(W):                                                                        # [B, n] -> [B]
        r = torch.einsum("brn,bn->br", A, W) - y
        return 0.5 * (r * r).sum(dim=1)

    stop = capi.default_stop("lbfgsb")
    stop.gradient_norm = 1e-6                      # the projected-gradient tolerance, and the only test that stops
    stop.f_delta, stop.x_delta, stop.past, stop.num_iterations = 0.0, 0.0, 0, 500
    box = amd.BatchedLbfgsb(m=5, stopping_progress=stop)
    box.SetBounds([0.0] * n, [10.0] * n)
    w, f, g, progress = box.minimize_callable(value, torch.full((B, n), 0.5, dtype=torch.float64, device="cuda:0"))
    torch.cuda.synchronize()
    p = amd.progress_to_numpy(progress)
    projected = torch.where((w <= 0.0) & (g > 0.0), torch.zeros_like(g), g)
    print("%d problems: statuses %s, iterations median %d max %d, evaluations max %d" % (
        B, {int(k): int(v) for k, v in zip(*np.unique(p["status"], return_counts=True))},
        int(np.median(p["num_iterations"])), int(p["num_iterations"].max()), int(p["nfev"].max())))
    print("min w %.3g (never below 0), weights on the bound %.1f %%, max projected gradient %.3g, max |w - w_true| %.3g"
          % (float(w.min()), 100.0 * float((w == 0.0).double().mean()), float(projected.abs().max()),
             float((w - w_true).abs().max())))


if __name__ == "__main__":
    main()
