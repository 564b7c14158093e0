"""The lean solve kernels (csrc/dispatch_lean.hip) against the general kernel they specialise.

The lean instantiation of lbfgs_solve_kernel fixes the launch options of a plain First-mode solve at compile time
(LeanOptions, csrc/lbfgs_kernel.hpp) and drops only scalar and control work; every fp64 operation stays where it was.  So
the two kernels must return EQUAL BITS in x, f, g and every progress field.  The general kernel is forced through an
option that disqualifies the lean one without changing a result: a trace of one problem.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROGRESS_FIELDS = ("status", "num_iterations", "nfev", "sum_k", "x_delta", "f_delta", "gradient_norm")


def _solve(s, x0_dev, n, force_general=False, objective=None):
    import torch
    import cppnumericalsolvers_amd as amd
    trace = amd.Trace([0], 4, n, x0_dev.device, with_x=False) if force_general else None
    x, f, g, p = s.minimize(objective or amd.Rosenbrock(), x0_dev, trace=trace)
    torch.cuda.synchronize()
    return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p), s.last_launch()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64) if a.dtype == np.float64 else a


def _assert_same_bits(lean, general):
    for name, a, b in zip(("x", "f", "g"), lean[:3], general[:3]):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=name)
    for k in PROGRESS_FIELDS:
        np.testing.assert_array_equal(_bits(lean[3][k]), _bits(general[3][k]), err_msg=k)


# configs[1] whole; a prefix of configs[2] (its first 32,768 start points); the ten-column kernel at 8 x 4 and the
# six-column kernel at 16 x 4, which the two flagship batches do not reach
@pytest.mark.parametrize("B,n,m,W,mr", [(65536, 32, 6, 8, 6), (32768, 64, 10, 16, 10), (4096, 32, 9, 8, 10),
                                        (4096, 64, 6, 16, 6)])
@pytest.mark.parametrize("stop_name", ["parity", "variant_a"])
def test_lean_kernel_equals_general_kernel_bitwise(B, n, m, W, mr, stop_name):
    import torch
    import cppnumericalsolvers_amd as amd
    if stop_name == "variant_a" and B > 4096:
        B = 4096
    stop = amd.parity_stop()
    if stop_name == "variant_a":
        stop.x_delta = 1e-9
    x0 = torch.from_numpy(amd.synthetic_x0_host(B, n, "std")).to("cuda:0")
    s = amd.BatchedLbfgs(m=m, stopping_progress=stop, device=0)
    lean = _solve(s, x0, n)
    general = _solve(s, x0, n, force_general=True)
    assert lean[4]["kernel"] == "lean" and general[4]["kernel"] == "general"
    for ll in (lean[4], general[4]):
        assert (ll["lanes_per_problem"], ll["elems_per_lane"], ll["y_columns_in_registers"]) == (W, 4, mr)
    assert s.last_arithmetic() == "fma"
    _assert_same_bits(lean, general)
    assert np.all(lean[3]["status"] >= 2)         # every solve stopped on a test (not the iteration limit, 1)
    assert lean[3]["num_iterations"].max() > 50   # ... after a real solve


def test_calls_outside_the_lean_options_take_the_general_kernel():
    """past = 3 (the reference's default preset), an enabled f_delta test, an absolute gradient test, a preconditioner, a
    trace, the exact arithmetic and a problem that does not fill its segment each take the general kernel."""
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi
    B, n, m = 512, 32, 6
    x0 = torch.from_numpy(amd.synthetic_x0_host(B, n, "std")).to("cuda:0")
    ctx = amd.Context(0)

    def kernel_of(stop=None, force_general=False, objective=None, x=x0, **kw):
        s = amd.BatchedLbfgs(m=m, stopping_progress=stop or amd.parity_stop(), context=ctx, **kw)
        out = _solve(s, x, x.shape[1], force_general=force_general, objective=objective)
        assert np.all(np.isfinite(out[1]))
        return out[4]["kernel"]

    assert kernel_of() == "lean"
    assert kernel_of(stop=capi.default_stop()) == "general"          # past = 3
    past = amd.parity_stop()
    past.past, past.past_delta = 3, 1e-12
    assert kernel_of(stop=past) == "general"
    fd = amd.parity_stop()
    fd.f_delta, fd.f_delta_violations = 1e-300, 1
    assert kernel_of(stop=fd) == "general"
    absolute = amd.parity_stop()
    absolute.gradient_norm_relative = 0
    assert kernel_of(stop=absolute) == "general"
    second = amd.Rosenbrock()
    second.hessian_diagonal = np.ones(n)                              # Second mode: constant diagonal preconditioner
    assert kernel_of(objective=second) == "general"
    assert kernel_of(force_general=True) == "general"                 # a trace
    assert kernel_of(arithmetic="exact") == "general"
    assert kernel_of(x=x0[:, :31].contiguous()) == "general"          # n = 31 does not fill the 8 x 4 segment
    assert kernel_of() == "lean"                                      # (and the report follows the launch, not the context)
