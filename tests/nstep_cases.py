"""Shapes, inputs and trajectories of the Newton and first-order step audit (tests/nstep_lib.py): tests/test_nstep_lib.py runs
every row on the CPU twins, tests/test_gpu_newton_steps_mpmath.py and tests/test_gpu_first_order_steps_mpmath.py on the device.

Batches of 24 with the 8 traced rows of tests/step_cases.py and its stop record (the relative gradient test at 1e-6, every
other test off); the iteration limit is 30 for the two Newton solvers and 40 for the two first-order ones, cut where the 200-bit
replay of a row would take more than a few seconds (LIMIT_OF: the shape stays).

A trajectory is x_0 .. x_T with the value and gradient of every iterate AND the per-iteration counts d nfev, d sum_k, which no
trace record carries: they come from prefix-limited solves of the 8 traced rows (iterate k is the result of the same solve
limited to k - 1 iterations), for the twins and for the device alike; the device's traced x must equal theirs bit for bit.

The shapes sit where these kernels can go wrong, not at the workload's size.
  trust region, Newton descent (n <= 64, one coordinate per lane, W in {8, 16, 32, 64}): n = 2, 7, 8, 9 (the first n that
    pads to 16), 17, 33 (pads to 64), 64; Rosenbrock from the `std` and `u2` starts, the diagonal quadratic of
    step_cases.diag_coefficients, the dense quartic SPD family of dense_cases.integers(31, n, rows=24) at n = 7, 16, 33; for
    the trust region the INDEFINITE family at n = 7, 16 (negative curvature must end CG on the boundary), one row with an
    initial radius of 2^-6 (the first steps end on the boundary crossing and the radius grows) and one with 2^7 (the full
    Newton step is rejected and retried).
  first order (n <= 256): n = 2, 7, 33, 100, 256, Rosenbrock and the diagonal quadratic, every built mapping that covers
    n = 33 (64 x 1, 64 x 2, 64 x 4) and n = 256 (64 x 4), ConjugatedGradientDescent under both settings of eval_trials.
"""
import hashlib

import numpy as np

import dense_cases
import hp_lib
import nstep_lib as Ns
import step_cases as Sc

B, TRACED = Sc.B, Sc.TRACED
NEWTON_LIMIT, FIRST_ORDER_LIMIT = 30, 40
ROSENBROCK, DIAG_QUADRATIC, DENSE = 0, 1, 101
PROLOGUE_NFEV = {"trust_region": 1, "newton_descent": 1, "conjugated_gradient": 2, "gradient_descent": 1}
SMALL_RADIUS, LARGE_RADIUS = 2.0 ** -6, 2.0 ** 7

# (objective, start, n, config)
NEWTON_SHAPES = (("rosenbrock", "std", 2, None), ("rosenbrock", "u2", 7, None), ("rosenbrock", "std", 8, None),
                 ("rosenbrock", "u2", 9, None), ("rosenbrock", "std", 17, None), ("rosenbrock", "u2", 33, None),
                 ("rosenbrock", "std", 64, None), ("diag_quadratic", "std", 7, None), ("diag_quadratic", "u2", 17, None),
                 ("diag_quadratic", "std", 64, None), ("dense", "spd", 7, None), ("dense", "spd", 16, None),
                 ("dense", "spd", 33, None))
TRUST_REGION_ONLY = (("dense", "indefinite", 7, None), ("dense", "indefinite", 16, None),
                     ("rosenbrock", "std", 9, (("initial_radius", SMALL_RADIUS),)),
                     ("rosenbrock", "u2", 8, (("initial_radius", LARGE_RADIUS),)))
FIRST_ORDER_SHAPES = (("rosenbrock", "std", 2, None), ("rosenbrock", "u2", 7, None), ("rosenbrock", "std", 33, None),
                      ("rosenbrock", "u2", 100, None), ("rosenbrock", "std", 256, None), ("diag_quadratic", "std", 7, None),
                      ("diag_quadratic", "u2", 33, None), ("diag_quadratic", "std", 100, None),
                      ("diag_quadratic", "u2", 256, None))
MAPPING_SHAPES = (("rosenbrock", "std", 33, None), ("rosenbrock", "std", 256, None))
# the built (lanes per problem, coordinates per lane) of the first-order kernels: one coordinate per lane at every width, two
# and four at 64 lanes
FIRST_ORDER_MAPPINGS = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4))
SOLVERS = ("trust_region", "newton_descent", "conjugated_gradient", "gradient_descent")


# Trust region on the dense SPD family at n = 16 and 33 (the only rows whose CG multiplies a full dense H at W = 16 and
# W = 64): S = diag(2^k) C diag(2^k) has a condition number of 1e5 there, CG-Steihaug runs towards its ten iterations from
# the fourth outer step on, and the running first-order bound through that many iterations of CG on such a matrix passes the
# curvature it has to sign (margin 4.4 inside slack 39 at iteration 4 of problem 0, n = 16; 427 inside 3190 at n = 33; under
# every seed from 1 to 13 and kappa = 8, 64, 512 alike).  One such decision ends a problem's audit, so these rows are steered
# by their limit and radius, not dropped: at the default radius the limit is 2 (three iterations, every one audited: CG ends
# on the boundary and on the tolerance, the radius grows), and n = 16 runs once more from initial_radius = 2^-6 under a
# limit of 4, where the first steps are short boundary steps of few CG iterations.
ROW_LIMITS = {("trust_region", ("dense", "spd", 16, None)): 2, ("trust_region", ("dense", "spd", 33, None)): 2,
              ("trust_region", ("dense", "spd", 16, (("initial_radius", SMALL_RADIUS),))): 4}
TRUST_REGION_ONLY += (("dense", "spd", 16, (("initial_radius", SMALL_RADIUS),)),)


def rows_of(solver):
    if solver == "trust_region":
        return NEWTON_SHAPES + TRUST_REGION_ONLY
    return NEWTON_SHAPES if solver == "newton_descent" else FIRST_ORDER_SHAPES


def mappings_of(n):
    """every built first-order mapping that covers n (as step_cases.mappings_of enumerates the Lbfgs ones)"""
    return [(W, E) for W, E in FIRST_ORDER_MAPPINGS if Sc.width(n) <= W * E <= 4 * Sc.width(n)]


def limit_of(solver, row):
    """the iteration limit of a row; the shape stays.  (ROW_LIMITS: the three dense SPD trust-region rows, above.)
    Time: the replay factorises a dense H at 200 bits once per Newton step and evaluates the definition twice per
    first-order step: the limit is 16 at n = 33 and 10 at n = 64 for the Newton solvers, 20 at n = 256 for the others.
    Trust region: 12.  From about the fifteenth outer step on Rosenbrock the forcing tolerance keeps CG running long enough
    for the running bound to pass a margin it has to decide (first undecidable decision under the limit of 30, reference
    order: iteration 15 at n = 7, 19 at n = 8, 27 at n = 9 and 17, 23 on the indefinite n = 16, 22 and 25 on the two radius
    rows), and one such decision ends a problem's audit: more than 2 % of a case.  Every problem is still audited through
    iteration 10, and every branch of the step runs in those iterations (required_branches)."""
    n = row[2]
    if (solver, row) in ROW_LIMITS:
        return ROW_LIMITS[(solver, row)]
    if solver in ("conjugated_gradient", "gradient_descent"):
        return FIRST_ORDER_LIMIT if n <= 100 else 20
    if solver == "trust_region":
        return 12 if n <= 33 else 10
    return NEWTON_LIMIT if n <= 17 else (16 if n <= 33 else 10)


def case_id(row):
    name, start, n, config = row
    return "%s-%s-%d%s" % (name, start, n, "".join("-%s=%g" % kv for kv in (config or ())))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def inputs(row, sequential=False):
    """(objective id, params blob or None, x0 [24, n], evaluate(x, hessian=False) -> hp_lib.Eval, (k_f, k_g, k_H))"""
    name, start, n, _ = row
    if name == "rosenbrock":
        k_f, k_g, k_H = hp_lib.rosenbrock_k(n)
        return (ROSENBROCK, None, Sc.starts(start, n), hp_lib.rosenbrock, ((n + 5) if sequential else k_f, k_g, k_H))
    if name == "diag_quadratic":
        a, c = Sc.diag_coefficients(n)
        k_f, k_g, k_H = hp_lib.diag_quadratic_k(n)
        return (DIAG_QUADRATIC, np.concatenate([a, [c]]), Sc.starts(start, n),
                (lambda x, hessian=False: hp_lib.diag_quadratic(x, a, c, hessian=hessian)),
                ((n + 3) if sequential else k_f, k_g, k_H))
    ints = dense_cases.integers(31, n, indefinite=(start == "indefinite"), rows=B)
    S, b, kappa = dense_cases.matrix(ints), ints["dense_bq"].astype(np.float64) / 64.0, float(ints["dense_kappa"])
    k_f, k_g, k_H = hp_lib.dense_quartic_k(n)
    # (the reference's order sums the value's n terms as a chain where the kernel has a tree)
    return (DENSE, dense_cases.params(ints), dense_cases.starts(ints),
            (lambda x, hessian=False: hp_lib.dense_quartic(x, S, b, kappa, hessian=hessian)),
            ((2 * n + 3) if sequential else k_f, k_g, k_H))


def rules_of(solver, row, family="exact"):
    return Ns.Rules(solver, dot="sequential" if family == "reference" else "tree", config=dict(row[3] or ()))


# ---- trajectories ------------------------------------------------------------------------------------------------------------
def prefix_trajectories(solve, x0, f0, g0, limit, prologue_nfev):
    """solve(x0 rows, stop fields) -> (x, f, g, progress) -> [(xs, gs, fs, dnfev, dsumk)] per row of x0: iterate k from the
    solve limited to k - 1 iterations (step_cases.prefix_trajectories), with what that iteration added to nfev and sum_k"""
    rows = x0.shape[0]
    out = [([x0[b]], [g0[b]], [f0[b]], [], []) for b in range(rows)]
    counts = [(prologue_nfev, 0)] * rows
    running = list(range(rows))
    for k in range(1, limit + 2):
        if not running:
            break
        x, f, g, p = solve(x0[running], Sc.first_iteration_fields() if k == 1 else Sc.stop_fields(k - 1))
        still = []
        for i, b in enumerate(running):
            done = int(p["num_iterations"][i])
            assert done <= k, "a solve limited to %d iterations took %d" % (k - 1, done)
            if done == k:
                nfev, sumk = int(p["nfev"][i]), int(p["sum_k"][i])
                out[b][0].append(x[i])
                out[b][1].append(g[i])
                out[b][2].append(f[i])
                out[b][3].append(nfev - counts[b][0])
                out[b][4].append(sumk - counts[b][1])
                counts[b] = (nfev, sumk)
                still.append(b)
            else:
                assert done == k - 1 and np.array_equal(x[i], out[b][0][-1]), "a prefix-limited solve took another path"
        running = still
    return [tuple(np.array(a) for a in t) for t in out]


def assert_trace_is_the_prefix_path(traced, prefixed, what):
    """the trace record of one launch against the prefix-limited launches: the same iterates, bit for bit"""
    assert len(traced) == len(prefixed)
    for i, ((tx, tg, tf), (px, pg, pf, _, _)) in enumerate(zip(traced, prefixed)):
        for name, a, b in (("x", tx, px), ("g", tg, pg), ("f", tf, pf)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), \
                "%s problem %d: the traced %s differs from the prefix-limited launches'" % (what, i, name)


_AUDITED = {}


def audit_once(trajectories, rules, evaluate, ks, what=""):
    """nstep_lib.audit_case, kept per trajectory: the kernels promise the same bits on every mapping, and the audit is a
    function of the trajectory and the rules alone"""
    h = hashlib.sha256(repr((rules.key(), tuple(ks))).encode())
    for t in trajectories:
        for a in t:
            h.update(np.ascontiguousarray(a).tobytes())
    key = h.hexdigest()
    if key not in _AUDITED:
        _AUDITED[key] = Ns.audit_case(trajectories, rules, evaluate, ks, what=what)
    return _AUDITED[key]


def assert_case(report, rules, what):
    """the bounds and the two caps; returns the report's line for the summary"""
    import step_lib
    line = "%s: %s" % (what, report.line())
    assert not report.bad, "%s\n%d outside their bound, first: %s" % (line, len(report.bad), report.bad[:3])
    broken = step_lib.caps(report, rules.m)
    assert not broken, "%s\n%s\nundecidable: %s\nexceptions: %s" % (line, broken, report.undecidable[:4],
                                                                       report.exception_notes[:4])
    return line


# ---- the branches a row must run (asserted on the reference-order twin and on the device) --------------------------------------
def required_branches(solver, row):
    """the counts that must be positive on a row.  Replayed, not exercised by any input: cg_zero (the early exit needs
    |g|_2 <= 0.25 |g|_inf, which no vector meets), no_promise of NewtonDescent (the fixed point of alpha * rho, 7,050
    trials), the refused search of GradientDescent (g.g = 0), and a first-order search that accepts its first trial
    (armijo_first: the unit step along -g or the Fletcher-Reeves direction overshoots on every row but three steps of
    GradientDescent at n = 2)."""
    name, start, n, config = row
    if solver == "trust_region":
        if start == "indefinite":
            return ("cg_negative",)
        if config and dict(config)["initial_radius"] == SMALL_RADIUS:
            return ("cg_boundary", "grows")
        if config and dict(config)["initial_radius"] == LARGE_RADIUS:
            return ("retries", "shrinks")
        if name == "diag_quadratic":         # convex, the unit radius binds at first; 17 and 64 distinct eigenvalues: the cap
            return ("cg_boundary", "grows") + (("cg_cap",) if n >= 17 else ("cg_tolerance",))
        if name == "dense":
            return ("cg_tolerance", "cg_boundary", "grows")
        return ("cg_tolerance", "cg_boundary", "cg_negative", "retries", "shrinks", "grows")
    if solver == "newton_descent":
        return ("armijo_first", "armijo_later") if name == "rosenbrock" else ("armijo_first",)
    return ("armijo_later",)


# ---- the device (tests/test_gpu_newton_steps_mpmath.py, tests/test_gpu_first_order_steps_mpmath.py) ---------------------------------
def device_objective(row):
    import cppnumericalsolvers_amd as amd
    oid, blob, _, _, _ = inputs(row)
    if oid == ROSENBROCK:
        return amd.Rosenbrock()
    if oid == DIAG_QUADRATIC:
        return amd.DiagQuadratic(blob[:-1], blob[-1])
    return amd.Objective(DENSE, blob, "dense_quartic")


def device_trajectories(make_solver, solver, row, after_launch=None, make_default=None):
    """One launch of the 24 problems with an amd.Trace of the 8 rows TRACED (x, g, f of every iterate), the device's own
    f(x_0), g(x_0), and the prefix-limited launches of those 8 rows for d nfev and d sum_k; the traced iterates must be the
    prefix-limited ones bit for bit.  make_solver(stop) -> a Batched* solver; make_default(stop) -> the same solver at the
    library's mapping, where make_solver asks for an explicit one (the evaluation entry takes the library's mapping or a
    complete (lanes, coordinates per lane) pair, not lanes alone)."""
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import capi

    def stop_of(fields):
        s = capi.Stop()
        for k, v in fields.items():
            setattr(s, k, v)
        return s

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    x0 = inputs(row)[2]
    n, limit = x0.shape[1], limit_of(solver, row)
    objective = device_objective(row)
    rows = list(TRACED)
    full = make_solver(stop_of(Sc.stop_fields(limit)))
    trace = amd.Trace(rows, capacity=limit + 2, n=n, device=full.device, with_x=True, with_g=True)
    full.minimize(objective, dev(x0), trace=trace)
    torch.cuda.synchronize()
    if after_launch:
        after_launch(full)
    evaluator = make_default(stop_of(Sc.stop_fields(limit))) if make_default else full
    f0, g0 = evaluator.evaluate(objective, dev(x0[rows]))
    torch.cuda.synchronize()
    f0, g0 = f0.cpu().numpy(), g0.cpu().numpy()
    traced = Sc.trace_trajectories(trace, x0[rows], f0, g0)

    def solve(part, fields):
        s = make_solver(stop_of(fields))
        x, f, g, p = s.minimize(objective, dev(part))
        torch.cuda.synchronize()
        return x.cpu().numpy(), f.cpu().numpy(), g.cpu().numpy(), amd.progress_to_numpy(p)

    prefixed = prefix_trajectories(solve, x0[rows], f0, g0, limit, PROLOGUE_NFEV[solver])
    assert_trace_is_the_prefix_path(traced, prefixed, "%s %s" % (solver, case_id(row)))
    return prefixed
