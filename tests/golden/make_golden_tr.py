"""Writes tests/golden/trust_region_reference_vectors.npz: TrustRegionNewton solves of the reference (its
solver/trust_region_newton.h over the Eigen stand-in, tests/trust_region/ref_harness.cpp compiled into a temporary
directory outside the tree).  Run by hand where the reference tree exists:  python tests/golden/make_golden_tr.py

Every case is a dict of arrays: objective, x0, params, stop, config, condition_stop and the reference's x, f, g, progress
(status, num_iterations, nfev, x_delta, f_delta, gradient_norm; CG iterations are not observable from outside it)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
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


def main():
    with tempfile.TemporaryDirectory() as d:
        lib = T.build_reference(d)
        ref = T.reference_solver(lib)
        arrays = {}
        for name, obj, x0, params, stop, cfg, cs in cases():
            st = T.make_stop(**(T.STOP_PRESETS[stop] if isinstance(stop, str) else stop))
            c = T.make_config(**cfg)
            x, f, g, p = ref(obj, x0, params, st, c, cs)
            rec = dict(objective=np.int32(obj), x0=x0, params=params if params is not None else np.zeros(1),
                       stop=st, config=c, condition_stop=np.float64(cs), x=x, f=f, g=g, progress=p)
            if x0.shape[0] == 1:
                # single-start cases (the example program, the scenarios): the states the reference's step callback sees
                # after every Progress::Update — trajectory rows (num_iterations, status, value, x_delta, f_delta,
                # gradient_norm) and the iterates
                tx, tf, tg, tp, rows, xs = T.reference_trajectory(lib, obj, x0, params, st, c, cs)
                assert tx.tobytes() == x.tobytes() and len(rows) == int(p["num_iterations"][0])
                rec.update(trajectory=rows, trajectory_x=xs)
            for k, v in rec.items():
                arrays[name + "/" + k] = v
        np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
