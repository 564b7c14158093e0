"""A float32 loss in plain torch ops, minimised in float32: B small robust regressions, one data set per problem.

    f_b(w) = sum_i huber(a_bi . w - y_bi) + 1/2 lambda ||w||^2          (Huber loss with delta = 1)

Data, model and loss are float32, torch's default dtype, and nothing is cast: BatchedLbfgs(dtype=torch.float32) runs the
native float solver (Lbfgs<F, m, MoreThuente> with ScalarType = float), minimize_callable hands the objective the
solver's float32 [B, n] buffer of trial points, and the gradient comes from autograd in float32.  The stopping
thresholds are float thresholds: a gradient test far below sqrt(eps_float) ~ 3e-4 of the loss's scale cannot fire.
Needs an MI355X.
    python examples/ask_tell/float32_objective.py [--problems 4096] [--rows 64] [--features 10]"""
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
    gen = torch.Generator().manual_seed(20261020)
    A = torch.randn(B, rows, n, generator=gen).to("cuda:0")                              # per-problem data, float32
    w_true = torch.randn(B, n, generator=gen).to("cuda:0")
    y = torch.einsum("brn,bn->br", A, w_true) + 0.1 * torch.randn(B, rows, generator=gen).to("cuda:0")
    y[:, ::8] += 5.0                                                                     # outliers

    def value(W):                                                                        # [B, n] float32 -> [B] float32
        r = torch.einsum("brn,bn->br", A, W) - y
        return torch.nn.functional.huber_loss(r, torch.zeros_like(r), reduction="none").sum(dim=1) + \
            0.5 * lam * (W * W).sum(dim=1)

    stop = capi.default_stop()
    stop.gradient_norm, stop.gradient_norm_relative, stop.past, stop.num_iterations = 1e-2, 1, 0, 200
    solver = amd.BatchedLbfgs(m=10, stopping_progress=stop, arithmetic="exact", dtype=torch.float32)
    w, f, g, progress = solver.minimize_callable(value, torch.zeros(B, n, device="cuda:0"))
    torch.cuda.synchronize()
    assert w.dtype == f.dtype == g.dtype == torch.float32
    p = amd.progress_to_numpy(progress)
    print("%d problems in float32: statuses %s, iterations median %d max %d, evaluations max %d, max ||g||inf %.3g, "
          "median |w - w_true|inf %.3g"
          % (B, {int(k): int(v) for k, v in zip(*np.unique(p["status"], return_counts=True))}, int(np.median(p["num_iterations"])),
             int(p["num_iterations"].max()), int(p["nfev"].max()), float(g.abs().max()),
             float((w - w_true).abs().amax(dim=1).median())))


if __name__ == "__main__":
    main()
