"""Writes tests/golden/newton_descent_reference_vectors.npz: NewtonDescent solves of the reference (its
solver/newton_descent.h and linesearch/armijo.h over the Eigen stand-in, tests/newton_descent/ref_harness.cpp compiled
into a temporary directory outside the tree).  Run by hand where the reference tree exists, after build():
    python tests/golden/make_golden_nd.py

Every case is a dict of arrays: objective, x0, params, stop, config, condition_stop, marked (nd_cases.py) and the
reference's x, f, g, progress (status, num_iterations, nfev, x_delta, f_delta, gradient_norm; the trial points are not
observable from outside it); single-start cases also hold the states the reference's step callback sees.  Every solve
caps num_iterations at 300 or less.  The assertions at the end come from counters the twin returns: if one fails, change
the starts, not the assertion."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nd_cases  # noqa: E402
import nd_lib as T  # noqa: E402

OUT = os.path.join(HERE, "newton_descent_reference_vectors.npz")
CAP = 300


def stop(preset, **kw):
    return {**T.STOP_PRESETS[preset], "num_iterations": CAP, **kw}


def starts(rng, n, B, scales):
    """x0 = 1 + s u, s drawn per row from `scales`, u uniform in [-1, 1] (the chained Rosenbrock's minimiser is 1)"""
    s = rng.choice(scales, size=B)
    return 1.0 + s[:, None] * rng.uniform(-1.0, 1.0, (B, n))


def cases():
    """(name, objective, x0, params, stop dict, condition_stop)"""
    rng = np.random.default_rng(20261018)
    out = []
    # the two scenarios of src/test/verify.cc (SOLVER_SETUP(NewtonDescent, RosenbrockFull)): the default stop
    out.append(("scenario_verify_far", T.ROSENBROCK, np.array([[15.0, 8.0]]), None, stop("default"), 0.0))
    out.append(("scenario_verify_near", T.ROSENBROCK, np.array([[-1.0, 2.0]]), None, stop("default"), 0.0))
    for n in (2, 7, 8, 9, 32, 33, 64):
        x0 = starts(rng, n, 8, (0.05, 0.5))
        for preset in ("default", "parity"):
            out.append(("rosenbrock_n%02d_%s" % (n, preset), T.ROSENBROCK, x0, None, stop(preset), 0.0))
    out.append(("rosenbrock_n08_stall", T.ROSENBROCK, starts(rng, 8, 8, (2.0, 3.0)), None, stop("default"), 0.0))
    for n in (5, 32):
        a = np.concatenate([rng.uniform(0.5, 3.0, n), [0.25]])
        out.append(("diag_quadratic_n%02d" % n, T.DIAG_QUADRATIC, rng.uniform(-2.0, 2.0, (8, n)), a, stop("default"), 0.0))
    out.append(("quartic_n01", T.QUARTIC, rng.uniform(-3.0, 3.0, (8, 1)), None, stop("default"), 0.0))
    out.append(("quartic_n03", T.QUARTIC, rng.uniform(-3.0, 3.0, (8, 3)), None, stop("default"), 0.0))
    out.append(("quartic_single", T.QUARTIC, np.array([[0.1]]), None, stop("default", gradient_norm=1e-10), 0.0))
    out.append(("edge_condition_hessian", T.ROSENBROCK, starts(rng, 4, 8, (0.5,)), None, stop("default"), 50.0))
    out.append(("edge_at_minimiser", T.ROSENBROCK, np.ones((2, 7)), None, stop("default"), 0.0))
    out.append(("edge_overflow", T.ROSENBROCK, np.full((2, 4), 1e100), None, stop("default"), 0.0))
    return out


def main():
    with tempfile.TemporaryDirectory() as d:
        lib = T.build_reference(d)
        ref = T.reference_solver(lib)
        arrays, marked_names, names = {}, [], []
        interchanges = max_trials = alpha_one = alpha_less = 0
        for name, obj, x0, params, st, cs in cases():
            st, c = T.make_stop(**st), T.make_config()
            assert 0 < int(st["num_iterations"][0]) <= CAP
            # the twin first: a solve that reaches the fixed point of alpha *= rho would not return from the reference
            twin = T.twin_solve(obj, x0, params, st, c, cs, order=T.REF_ORDER, counters=True)
            cnt = twin[4]
            assert (cnt["fixed_point"] == 0).all(), name + ": a recorded solve reached the fixed point of alpha"
            dev = T.twin_solve(obj, x0, params, st, c, cs, order=T.DEVICE_ORDER)
            marked = bool(nd_cases.misses_contract(twin, dev).any())
            x, f, g, p = ref(obj, x0, params, st, c, cs)
            interchanges += int(cnt["interchanges"].sum())
            max_trials = max(max_trials, int(cnt["max_trials"].max()))
            alpha_one += int(cnt["alpha_one_steps"].sum())
            alpha_less += int(cnt["alpha_less_steps"].sum())
            print("%-28s status %-10s it %-10s max trials %4d interchanges %4d%s"
                  % (name, sorted(set(p["status"].tolist())), (p["num_iterations"].min(), p["num_iterations"].max()),
                     cnt["max_trials"].max(), cnt["interchanges"].sum(), "  MARKED" if marked else ""))
            names.append(name)
            if marked:
                marked_names.append(name)
            rec = dict(objective=np.int32(obj), x0=x0, params=params if params is not None else np.zeros(1),
                       stop=st, config=c, condition_stop=np.float64(cs), marked=np.int32(marked), x=x, f=f, g=g,
                       progress=p)
            if x0.shape[0] == 1:
                tx, tf, tg, tp, rows, xs = T.reference_trajectory(lib, obj, x0, params, st, c, cs, capacity=CAP + 1)
                assert tx.tobytes() == x.tobytes() and len(rows) == int(p["num_iterations"][0])
                rec.update(trajectory=rows, trajectory_x=xs)
            for k, v in rec.items():
                arrays[name + "/" + k] = v
        assert interchanges >= 1, "no recorded solve performed a row interchange in the LU"
        assert max_trials >= 100, "no step took at least 100 trials (longest %d)" % max_trials
        assert alpha_one >= 1 and alpha_less >= 1, "alpha = 1 and alpha < 1 must both be accepted somewhere"
        assert len(marked_names) <= nd_cases.MAX_MARKED_FRACTION * len(names), marked_names
        assert not [m for m in marked_names if m.startswith(nd_cases.NEVER_MARKED)], marked_names
        np.savez_compressed(OUT, **arrays)
    print("marked:", marked_names)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
