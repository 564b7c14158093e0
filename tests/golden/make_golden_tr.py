"""Writes tests/golden/trust_region_reference_vectors.npz: TrustRegionNewton solves of the reference (its
solver/trust_region_newton.h over the Eigen stand-in, tests/trust_region/ref_harness.cpp compiled into a temporary
directory outside the tree).  Run by hand where the reference tree exists:  python tests/golden/make_golden_tr.py

Every case is a dict of arrays: objective, x0, params, stop, config, condition_stop and the reference's x, f, g, progress
(status, num_iterations, nfev, x_delta, f_delta, gradient_norm; CG iterations are not observable from outside it).

The dense-Hessian cases (dense_..., objective 101, tests/dense_cases.py) are kept as the integers they are built from,
x* in full up to n = 33 and as a digest above, g* as a digest.  This file marks no case, so a dense case keeps only the
starts on which the twin's two summation orders meet the contract (x*, f* within 1e-6, equal status), at least 4 of the
8 drawn.  The assertions of dense_assertions() come from the twin's counters: if one fails, change the inputs, not the
assertion."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dense_cases as D  # noqa: E402
import nd_cases  # noqa: E402
import tr_lib as T  # noqa: E402

OUT = os.path.join(HERE, "trust_region_reference_vectors.npz")


def cases():
    """(name, objective, x0, params, stop preset / dict, config overrides, condition_stop)"""
    rng = np.random.default_rng(20261016)
    out = []
    for n in (1, 2, 7, 32, 64):
        for preset in ("default", "conservative", "parity"):
            out.append(("rosenbrock_n%d_%s" % (n, preset), T.ROSENBROCK, rng.uniform(-2.0, 2.0, (8, n)), None, preset, {},
                        0.0))
    a = np.concatenate([rng.uniform(0.5, 3.0, 12), [0.25]])
    out.append(("diag_quadratic_convex", T.DIAG_QUADRATIC, rng.uniform(-2.0, 2.0, (8, 12)), a, "default", {}, 0.0))
    a = np.concatenate([rng.uniform(-3.0, 3.0, 12), [1.0]])
    a[0], a[1] = -1.5, 2.0    # indefinite for sure: unbounded below, ends at the iteration limit
    out.append(("diag_quadratic_indefinite", T.DIAG_QUADRATIC, rng.uniform(-2.0, 2.0, (8, 12)), a,
                {**T.STOP_PRESETS["default"], "num_iterations": 25}, {}, 0.0))
    out.append(("quartic", T.QUARTIC, rng.uniform(-3.0, 3.0, (16, 1)), None, "default", {}, 0.0))
    # edge configurations
    out.append(("edge_at_minimiser", T.ROSENBROCK, np.ones((2, 7)), None, "default", {}, 0.0))
    out.append(("edge_retry_limit_0", T.ROSENBROCK, rng.uniform(-2.0, 2.0, (4, 7)), None, "default",
                dict(rejection_retry_limit=0), 0.0))
    out.append(("edge_cg_floor_0", T.ROSENBROCK, rng.uniform(-2.0, 2.0, (4, 7)), None, "default",
                dict(cg_max_iterations_floor=0), 0.0))
    out.append(("edge_tight_max_radius", T.ROSENBROCK, rng.uniform(-2.0, 2.0, (4, 7)), None, "default",
                dict(max_radius=0.05), 0.0))
    out.append(("edge_min_radius_stall", T.ROSENBROCK, rng.uniform(-2.0, 2.0, (4, 7)), None, "default",
                dict(min_radius=0.5), 0.0))
    out.append(("edge_overflow_trial", T.ROSENBROCK, np.full((2, 4), 1e100), None, "default", {}, 0.0))
    out.append(("edge_condition_hessian", T.ROSENBROCK, rng.uniform(-2.0, 2.0, (8, 4)), None, "default", {}, 50.0))
    # the example program src/examples/trust_region_newton_rosenbrock.cc: Rosenbrock-2 from (-1.2, 1)
    out.append(("example_rosenbrock2", T.ROSENBROCK, np.array([[-1.2, 1.0]]), None,
                {**T.STOP_PRESETS["default"], "gradient_norm": 1e-10, "num_iterations": 200}, {}, 0.0))
    # the eight scenarios of src/test/trust_region_newton_test.cc (default stopping progress with the fields each sets;
    # its quadratics are DiagQuadratic: 3 x0^2 + 10 x1^2 and 0.5 (x0^2 - x1^2))
    convex, saddle = np.array([3.0, 10.0, 0.0]), np.array([0.5, -0.5, 0.0])

    def stop(**kw):
        return {**T.STOP_PRESETS["default"], **kw}
    out += [
        ("scenario_strictly_convex_quadratic", T.DIAG_QUADRATIC, np.array([[10.0, -5.0]]), convex,
         stop(gradient_norm=1e-10, num_iterations=20), {}, 0.0),
        ("scenario_rosenbrock_standard_start", T.ROSENBROCK, np.array([[-1.2, 1.0]]), None,
         stop(gradient_norm=1e-8, num_iterations=200), {}, 0.0),
        ("scenario_boundary_exit_radius", T.DIAG_QUADRATIC, np.array([[5.0, 5.0]]), convex,
         stop(gradient_norm=0.0, num_iterations=5), dict(initial_radius=0.5), 0.0),
        ("scenario_indefinite_bounded_step", T.DIAG_QUADRATIC, np.array([[0.1, 0.5]]), saddle,
         stop(gradient_norm=0.0, num_iterations=5), dict(initial_radius=1.0), 0.0),
        ("scenario_interior_newton_step", T.DIAG_QUADRATIC, np.array([[1.0, 1.0]]), convex,
         stop(gradient_norm=1e-12, num_iterations=5), dict(initial_radius=100.0), 0.0),
        ("scenario_quartic_double_well", T.QUARTIC, np.array([[0.1]]), None,
         stop(gradient_norm=1e-10, num_iterations=100), dict(initial_radius=0.5), 0.0),
        ("scenario_max_radius_cap", T.DIAG_QUADRATIC, np.array([[100.0, -100.0]]), convex,
         stop(gradient_norm=1e-10, num_iterations=200), dict(initial_radius=0.5, max_radius=2.0), 0.0),
        ("scenario_gradient_norm_stop", T.DIAG_QUADRATIC, np.array([[3.0, 3.0]]), convex,
         stop(gradient_norm=1e-4, num_iterations=100), {}, 0.0),
        ("scenario_iteration_limit_stop", T.ROSENBROCK, np.array([[-1.2, 1.0]]), None,
         stop(gradient_norm=1e-16, num_iterations=1), {}, 0.0),
    ]
    return out


# seed per dimension of the dense families (dense_cases.integers), as the Newton-descent file uses them
DENSE_SEEDS = {2: 2, 3: 1, 7: 1, 8: 1, 9: 34, 16: 15, 17: 19, 32: 12, 33: 101, 63: 17, 64: 13}
# the condition stop: (n, threshold, rows of the SPD case's starts) — rows that end on it after a few steps and rows whose
# condition numbers stay below it
DENSE_CONDITION = ((9, 603.0, (0, 1, 3, 6)), (33, 42758.0, (0, 1, 2, 4)), (64, 600000.0, (1, 4, 6, 7)))


def _rows(ints, rows):
    return {**ints, "x0_q": np.ascontiguousarray(ints["x0_q"][list(rows)])}


def dense_cases():
    """(name, integers, stop preset, condition_stop)"""
    out = []
    for n in D.DIMS:
        spd = D.integers(DENSE_SEEDS[n], n)
        for preset in ("default", "parity"):
            out.append(("dense_spd_n%02d_%s" % (n, preset), spd, preset, 0.0))
        out.append(("dense_asym_n%02d_default" % n, D.integers(DENSE_SEEDS[n], n, flags=D.ASYMMETRIC), "default", 0.0))
        out.append(("dense_indefinite_n%02d_default" % n, D.integers(DENSE_SEEDS[n], n, indefinite=True), "default", 0.0))
    for n, threshold, rows in DENSE_CONDITION:
        out.append(("dense_condition_n%02d" % n, _rows(D.integers(DENSE_SEEDS[n], n), rows), "default", threshold))
    # a single start: the reference's callback states go with it
    out.append(("dense_single_n17", _rows(D.integers(DENSE_SEEDS[17], 17), (0,)), "default", 0.0))
    return out


def within_contract(ints, st, c, cs):
    """The case with the starts dropped on which the twin's two orders miss the contract."""
    args = (D.DENSE, D.starts(ints), D.params(ints), st, c, cs)
    keep = ~nd_cases.misses_contract(T.twin_solve(*args, order=T.REF_ORDER), T.twin_solve(*args, order=T.DEVICE_ORDER))
    return _rows(ints, np.nonzero(keep)[0])


def dense_assertions(counters, progress, inputs):
    assert any(counters["dense_spd_n%02d_%s" % (n, preset)]["max_cg_iterations"].max() >= 3
               for n in D.DIMS if n >= 33 for preset in ("default", "parity")), "no step at n >= 33 ran 3 CG iterations"
    indefinite = [k for k in counters if k.startswith("dense_indefinite_")]
    assert sum(int(counters[k]["negative_curvature_exits"].sum()) for k in indefinite) >= 1
    assert sum(int(counters[k]["boundary_hits"].sum()) for k in indefinite) >= 1
    for name, case in inputs.items():
        assert case["x0"].shape[0] >= (4 if not name.startswith("dense_single_") else 1), name
        args = (D.DENSE, case["x0"], case["params"], case["stop"], case["config"], float(case["condition_stop"]))
        ref_order, dev_order = T.twin_solve_ex(*args, order=T.REF_ORDER), T.twin_solve_ex(*args, order=T.DEVICE_ORDER)
        assert not nd_cases.misses_contract(ref_order, dev_order).any(), name
        if name.startswith("dense_condition_"):
            status = progress[name]["status"]
            assert min(ref_order[4]["min_condition_margin"].min(), dev_order[4]["min_condition_margin"].min()) >= 1e-9, name
            assert (status == 5).any() and (status != 5).any(), (name, status)
            assert (progress[name]["num_iterations"][status == 5] >= 2).any(), name
        if name.startswith("dense_asym_"):
            # the planted bug (H d walking a column of H for a row) changes the bytes of every asymmetric case
            assert D.tr_transposition_shows(case), name


def main():
    with tempfile.TemporaryDirectory() as d:
        lib = T.build_reference(d)
        ref = T.reference_solver(lib)
        arrays, dense_arrays, counters, progress, inputs, cg_iterations = {}, {}, {}, {}, {}, {}
        everything = [(nm, obj, x0, params, stop, cfg, cs, None) for nm, obj, x0, params, stop, cfg, cs in cases()] + \
                     [(nm, D.DENSE, None, None, stop, {}, cs, ints) for nm, ints, stop, cs in dense_cases()]
        for name, obj, x0, params, stop, cfg, cs, ints in everything:
            st = T.make_stop(**(T.STOP_PRESETS[stop] if isinstance(stop, str) else stop))
            c = T.make_config(**cfg)
            if ints is not None:
                if not name.startswith(("dense_condition_", "dense_single_")):
                    ints = within_contract(ints, st, c, cs)
                x0, params = D.starts(ints), D.params(ints)
            x, f, g, p = ref(obj, x0, params, st, c, cs)
            if ints is None:
                rec = dict(objective=np.int32(obj), x0=x0, params=params if params is not None else np.zeros(1),
                           stop=st, config=c, condition_stop=np.float64(cs), x=x, f=f, g=g, progress=p)
            else:
                twin = T.twin_solve_ex(obj, x0, params, st, c, cs)
                assert twin[0].tobytes() == x.tobytes(), name     # (digests: see dense_cases.reference_x)
                counters[name], progress[name], cg_iterations[name] = twin[4], p, int(twin[3]["sum_k"].sum())
                inputs[name] = dict(x0=x0, params=params, stop=st, config=c, condition_stop=cs)
                print("%-32s rows %d status %-8s it %-10s max cg %2d negative curvature %3d boundary %3d"
                      % (name, len(x0), sorted(set(p["status"].tolist())),
                         (p["num_iterations"].min(), p["num_iterations"].max()), twin[4]["max_cg_iterations"].max(),
                         twin[4]["negative_curvature_exits"].sum(), twin[4]["boundary_hits"].sum()))
                rec = dict(objective=np.int32(obj), **ints, params_sha256=D.sha256(params), stop=st, config=c,
                           condition_stop=np.float64(cs), f=f, progress=p)
                D.record_results(rec, x, g)
            if x0.shape[0] == 1:
                # single-start cases (the example program, the scenarios): the states the reference's step callback sees
                # after every Progress::Update — trajectory rows (num_iterations, status, value, x_delta, f_delta,
                # gradient_norm) and the iterates
                tx, tf, tg, tp, rows, xs = T.reference_trajectory(lib, obj, x0, params, st, c, cs)
                assert tx.tobytes() == x.tobytes() and len(rows) == int(p["num_iterations"][0])
                rec.update(trajectory=rows, trajectory_x=xs)
            for k, v in rec.items():
                (arrays if ints is None else dense_arrays)[name + "/" + k] = v
        dense_assertions(counters, progress, inputs)
        print("dense: CG iterations %d over %d solves (longest subproblem %d, %d subproblems of 3 or more); negative "
              "curvature exits %d, boundary hits %d"
              % (sum(cg_iterations.values()), sum(len(progress[k]) for k in progress),
                 max(int(v["max_cg_iterations"].max()) for v in counters.values()),
                 sum(int(v["subproblems_of_3_cg_iterations"].sum()) for v in counters.values()),
                 sum(int(v["negative_curvature_exits"].sum()) for v in counters.values()),
                 sum(int(v["boundary_hits"].sum()) for v in counters.values())))
        np.savez_compressed(OUT, **arrays, **D.pack(dense_arrays))
    assert os.path.getsize(OUT) <= 260170, "the file may not outgrow the largest golden file"
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
