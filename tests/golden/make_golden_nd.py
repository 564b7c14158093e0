"""Writes tests/golden/newton_descent_reference_vectors.npz: NewtonDescent solves of the reference (its
solver/newton_descent.h and linesearch/armijo.h over the Eigen stand-in, tests/newton_descent/ref_harness.cpp compiled
into a temporary directory outside the tree).  Run by hand where the reference tree exists, after build():
    python tests/golden/make_golden_nd.py

Every case is a dict of arrays: objective, x0, params, stop, config, condition_stop, marked (nd_cases.py) and the
reference's x, f, g, progress (status, num_iterations, nfev, x_delta, f_delta, gradient_norm; the trial points are not
observable from outside it); single-start cases also hold the states the reference's step callback sees.  Every solve
caps num_iterations at 300 or less.  The assertions at the end come from counters the twin returns: if one fails, change
the starts, not the assertion.

The dense-Hessian cases (dense_..., objective 101, tests/dense_cases.py) are kept as the integers they are built from,
x* in full up to n = 33 and as a digest above, g* as a digest.  Their seeds were picked so that the assertions of
dense_assertions() hold: the LU's pivot search has to reach far rows, cross the 8-wide chunks and meet exact ties, and
the asymmetric variant has to tell a transposed read from the right one."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dense_cases as D  # noqa: E402
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


# seed per dimension of the dense families (dense_cases.integers): the first that meets dense_assertions()
DENSE_SEEDS = {2: 2, 3: 1, 7: 1, 8: 1, 9: 34, 16: 15, 17: 19, 32: 12, 33: 101, 63: 17, 64: 13}
# the condition stop: (n, threshold, rows of the SPD case's starts) — a threshold between the condition numbers the
# iterates pass through, so that rows end on it after one, two or three steps and others never do
DENSE_CONDITION = ((9, 600.0, (0, 1, 2, 3)), (33, 11000.0, (2, 4, 6, 7)), (64, 77000.0, (0, 3, 4, 7)))


def _rows(ints, rows):
    return {**ints, "x0_q": np.ascontiguousarray(ints["x0_q"][list(rows)])}


def dense_cases():
    """(name, integers, stop dict, condition_stop)"""
    out = []
    for n in D.DIMS:
        spd = D.integers(DENSE_SEEDS[n], n)
        for preset in ("default", "parity"):
            out.append(("dense_spd_n%02d_%s" % (n, preset), spd, stop(preset), 0.0))
        out.append(("dense_asym_n%02d_default" % n, D.integers(DENSE_SEEDS[n], n, flags=D.ASYMMETRIC), stop("default"), 0.0))
    out.append(("dense_indefinite_n09_default", D.integers(1, 9, indefinite=True, rows=4), stop("default"), 0.0))
    # kappa = 0: H = S is constant and full steps alone lead to the solution of S x = b; each leaves 1e-5 / lambda_min of
    # the error behind (the safe_guard), so the parity stop, and a seed whose S is conditioned well enough for 1e-6
    out.append(("dense_kappa0_n17", D.integers(27, 17, rows=3, kappa=0.0), stop("parity"), 0.0))
    for n, threshold, rows in DENSE_CONDITION:
        out.append(("dense_condition_n%02d" % n, _rows(D.integers(DENSE_SEEDS[n], n), rows), stop("default"), threshold))
    # a single start: the reference's callback states go with it
    out.append(("dense_single_n17", _rows(D.integers(DENSE_SEEDS[17], 17), (0,)), stop("default"), 0.0))
    return out


def dense_assertions(counters, progress, inputs):
    """Section by section what the dense inputs must reach, from the reference-order twin's counters per case."""
    def hist(name):
        return counters[name]["pivot_distance"].sum(axis=0)
    for n in D.DIMS:
        h = hist("dense_spd_n%02d_default" % n)
        if n >= 33:
            assert h[8:].sum() >= 100 and h[32:].sum() >= 10, (n, h[8:].sum(), h[32:].sum())
        if n in (8, 9):
            assert h[2:].sum() >= 10, (n, h[2:].sum())
    assert any(counters["dense_spd_n%02d_default" % n]["pivot_ties"].sum() >= 1 for n in D.DIMS if n >= 9), \
        "no pivot search met an exact tie"
    dense = [k for k in counters if k.startswith("dense_")]
    assert sum(int(counters[k]["alpha_one_steps"].sum()) for k in dense) >= 1
    assert sum(int(counters[k]["alpha_less_steps"].sum()) for k in dense) >= 1
    for n, _, _ in DENSE_CONDITION:
        name = "dense_condition_n%02d" % n
        c = inputs[name]
        device_order = T.twin_solve(D.DENSE, c["x0"], c["params"], c["stop"], c["config"], c["condition_stop"],
                                    order=T.DEVICE_ORDER, counters=True)[4]
        assert min(counters[name]["min_condition_margin"].min(), device_order["min_condition_margin"].min()) >= 1e-9, name
        status = progress[name]["status"]
        assert (status == 5).any() and (status != 5).any(), (name, status)
        assert (progress[name]["num_iterations"][status == 5] >= 2).any(), name + ": no row crosses the threshold mid-solve"
    # kappa = 0: full steps only, and no more than three of them
    assert (counters["dense_kappa0_n17"]["alpha_less_steps"] == 0).all()
    assert (progress["dense_kappa0_n17"]["num_iterations"] <= 3).all()
    # the zero column (device against twin only: the reference's safe_guard is a constant 1e-5)
    z = D.zero_column_case()
    cnt = T.twin_solve(D.DENSE, z["x0"], z["params"], z["stop"], z["config"], 0.0, counters=True)[4]
    assert (cnt["zero_columns"] >= 1).all() and (cnt["fixed_point"] == 0).all()
    # the chain of the search walking a row of H for a column changes the bytes of the strongly asymmetric cases (device
    # against twin only), and there the search shortens some step
    for n in D.CHAIN_CASES:
        z = D.chain_case(n)
        assert D.nd_mutation_shows(T.CHAIN_WALKS_ROW, z), z["name"]
        for order in (T.REF_ORDER, T.DEVICE_ORDER):
            out = T.twin_solve(D.DENSE, z["x0"], z["params"], z["stop"], z["config"], 0.0, order=order, counters=True)
            assert np.isfinite(out[0]).all() and (out[4]["alpha_less_steps"] >= 1).any(), z["name"]
    # H transposed before the LU changes the bytes of every asymmetric case
    for name in dense:
        if name.startswith("dense_asym_"):
            assert D.nd_transposition_shows(inputs[name]), name


def main():
    with tempfile.TemporaryDirectory() as d:
        lib = T.build_reference(d)
        ref = T.reference_solver(lib)
        arrays, dense_arrays, marked_names, names = {}, {}, [], []
        interchanges = max_trials = alpha_one = alpha_less = 0
        counters, progress, inputs = {}, {}, {}
        everything = [(nm, obj, x0, params, st, cs, None) for nm, obj, x0, params, st, cs in cases()] + \
                     [(nm, D.DENSE, D.starts(ints), D.params(ints), st, cs, ints) for nm, ints, st, cs in dense_cases()]
        for name, obj, x0, params, st, cs, ints in everything:
            st, c = T.make_stop(**st), T.make_config()
            assert 0 < int(st["num_iterations"][0]) <= CAP
            # the twin first: a solve that reaches the fixed point of alpha *= rho would not return from the reference
            twin = T.twin_solve(obj, x0, params, st, c, cs, order=T.REF_ORDER, counters=True)
            cnt = twin[4]
            assert (cnt["fixed_point"] == 0).all(), name + ": a recorded solve reached the fixed point of alpha"
            dev = T.twin_solve(obj, x0, params, st, c, cs, order=T.DEVICE_ORDER)
            marked = bool(nd_cases.misses_contract(twin, dev).any())
            x, f, g, p = ref(obj, x0, params, st, c, cs)
            counters[name], progress[name] = cnt, p
            inputs[name] = dict(x0=x0, params=params, stop=st, config=c, condition_stop=cs)
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
            if ints is None:
                rec = dict(objective=np.int32(obj), x0=x0, params=params if params is not None else np.zeros(1),
                           stop=st, config=c, condition_stop=np.float64(cs), marked=np.int32(marked), x=x, f=f, g=g,
                           progress=p)
            else:
                assert T.twin_solve(obj, x0, params, st, c, cs)[0].tobytes() == x.tobytes(), name   # (digests: see reference_x)
                rec = dict(objective=np.int32(obj), **ints, params_sha256=D.sha256(params), stop=st, config=c,
                           condition_stop=np.float64(cs), marked=np.int32(marked), f=f, progress=p)
                D.record_results(rec, x, g)
            if x0.shape[0] == 1:
                tx, tf, tg, tp, rows, xs = T.reference_trajectory(lib, obj, x0, params, st, c, cs, capacity=CAP + 1)
                assert tx.tobytes() == x.tobytes() and len(rows) == int(p["num_iterations"][0])
                rec.update(trajectory=rows, trajectory_x=xs)
            for k, v in rec.items():
                (arrays if ints is None else dense_arrays)[name + "/" + k] = v
        dense_assertions(counters, progress, inputs)
        hist = sum(counters[nm]["pivot_distance"].sum(axis=0) for nm, _, _, _ in dense_cases())
        print("dense: pivot distance 0: %d, 1: %d, >= 2: %d, >= 8: %d, >= 32: %d; ties %d; alpha = 1: %d, alpha < 1: %d"
              % (hist[0], hist[1], hist[2:].sum(), hist[8:].sum(), hist[32:].sum(),
                 sum(int(counters[nm]["pivot_ties"].sum()) for nm, _, _, _ in dense_cases()),
                 sum(int(counters[nm]["alpha_one_steps"].sum()) for nm, _, _, _ in dense_cases()),
                 sum(int(counters[nm]["alpha_less_steps"].sum()) for nm, _, _, _ in dense_cases())))
        assert interchanges >= 1, "no recorded solve performed a row interchange in the LU"
        assert max_trials >= 100, "no step took at least 100 trials (longest %d)" % max_trials
        assert alpha_one >= 1 and alpha_less >= 1, "alpha = 1 and alpha < 1 must both be accepted somewhere"
        assert len(marked_names) <= nd_cases.MAX_MARKED_FRACTION * len(names), marked_names
        assert not [m for m in marked_names if m.startswith(nd_cases.NEVER_MARKED)], marked_names
        np.savez_compressed(OUT, **arrays, **D.pack(dense_arrays))
    assert os.path.getsize(OUT) <= 260170, "the file may not outgrow the largest golden file"
    print("marked:", marked_names)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
