"""A loss with about a thousand parameters per problem, written in plain torch ops, values only: B small two-layer
networks, one data set each, fitted at once.

    f_b(w) = mean_i (W2_b . tanh(W1_b a_bi + c1_b) + c2_b - y_bi)^2 + 1/2 lambda ||w||^2,   w = (W1, c1, W2, c2)

With 24 inputs and 38 hidden units a problem has n = 24 * 38 + 38 + 38 + 1 = 989 parameters — more than the 256 a
wavefront segment holds, so BatchedLbfgs.minimize_callable runs the workgroup-per-problem ask/tell handle
(mi355_lbfgs_ask_tell_wide_*): nothing is compiled, the objective returns the values alone and the gradient comes from
autograd (the problems are independent, so the gradient of the sum is the per-problem gradient).  compact_every=16
drops finished problems from the evaluation every sixteen rounds; the objective indexes its data by `ids` then.
Needs an MI355X.
    python examples/ask_tell/wide_objective.py [--problems 256] [--rows 200] [--inputs 24] [--hidden 38]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--inputs", type=int, default=24)
    ap.add_argument("--hidden", type=int, default=38)
    args = ap.parse_args()
    import numpy as np
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi

    B, rows, d, h, lam = args.problems, args.rows, args.inputs, args.hidden, 1e-3
    n = d * h + h + h + 1
    gen = torch.Generator().manual_seed(20261021)
    A = torch.randn(B, rows, d, generator=gen, dtype=torch.float64).to("cuda:0")          # per-problem data
    y = torch.sin(A[:, :, 0]) + 0.5 * A[:, :, 1] * A[:, :, 2] + 0.05 * torch.randn(B, rows, generator=gen, dtype=torch.float64).to("cuda:0")

    def value(W, ids=None):                                                               # [rows, n] -> [rows]
        a, t = (A, y) if ids is None else (A[ids], y[ids])
        W1 = W[:, :d * h].reshape(-1, h, d)
        c1, W2, c2 = W[:, d * h:d * h + h], W[:, d * h + h:d * h + 2 * h], W[:, -1]
        hidden = torch.tanh(torch.einsum("bhd,brd->brh", W1, a) + c1[:, None, :])
        r = torch.einsum("brh,bh->br", hidden, W2) + c2[:, None] - t
        return (r * r).mean(dim=1) + 0.5 * lam * (W * W).sum(dim=1)

    stop = capi.default_stop()
    stop.gradient_norm, stop.gradient_norm_relative, stop.past, stop.num_iterations = 1e-5, 1, 0, 300
    solver = amd.BatchedLbfgs(m=10, stopping_progress=stop, arithmetic="exact")
    w0 = 0.3 * torch.randn(B, n, generator=gen, dtype=torch.float64).to("cuda:0")
    f0 = value(w0)
    w, f, g, progress = solver.minimize_callable(value, w0, compact_every=16)
    torch.cuda.synchronize()
    p = amd.progress_to_numpy(progress)
    print("%d problems of n = %d parameters: loss %.4f -> %.4f (medians), statuses %s, iterations median %d max %d, "
          "evaluations max %d, max ||g||inf %.3g"
          % (B, n, float(f0.median()), float(f.median()),
             {int(k): int(v) for k, v in zip(*np.unique(p["status"], return_counts=True))},
             int(np.median(p["num_iterations"])), int(p["num_iterations"].max()), int(p["nfev"].max()), float(g.abs().max())))


if __name__ == "__main__":
    main()
