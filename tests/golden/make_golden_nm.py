"""Writes tests/golden/nelder_mead_reference_vectors.npz: NelderMead solves of the reference (its solver/nelder_mead.h
over the Eigen stand-in with the column arithmetic of tests/nelder_mead/overlay, tests/nelder_mead/ref_harness.cpp
compiled into a temporary directory outside the tree).  Run by hand where the reference tree exists, after build():
    python tests/golden/make_golden_nm.py

Every case is a dict of arrays: objective, x0, params, stop, config (mode inside) and the reference's x, f, g, progress
(status, num_iterations, nfev, x_delta, f_delta, gradient_norm); single-start cases also hold the states the reference's
step callback sees.  Every solve caps num_iterations at 300 or less.  The reference orders equal vertex values as its
std::sort happens to, the project by the lower vertex index: the twin tells which solves met such a tie, and the cap of
nm_cases.MAX_TIED_FRACTION per case is asserted here — if a draw exceeds it, change the draw, not the cap."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nm_cases  # noqa: E402
import nm_lib as T  # noqa: E402

OUT = os.path.join(HERE, "nelder_mead_reference_vectors.npz")
CAP = 300


def stop(preset, **kw):
    return {**T.STOP_PRESETS[preset], "num_iterations": CAP, **kw}


def cases():
    """(name, objective, x0, params, stop dict, config overrides)"""
    rng = np.random.default_rng(20261017)
    out = []
    for n in (2, 3, 7, 8, 9, 16, 17, 32, 33, 64):
        x0 = rng.uniform(-2.0, 2.0, (8, n))
        for preset in ("solver", "default"):   # x_delta_violations 5 and 1
            out.append(("rosenbrock_n%02d_%s_value" % (n, preset), T.ROSENBROCK, x0, None, stop(preset), {}))
            if n <= 9:
                out.append(("rosenbrock_n%02d_%s_first" % (n, preset), T.ROSENBROCK, x0, None, stop(preset),
                            dict(mode=T.FIRST)))
    for n in (1, 12):
        a = np.concatenate([rng.uniform(0.5, 3.0, n), [0.25]])
        x0 = rng.uniform(-2.0, 2.0, (8, n))
        out.append(("diag_quadratic_n%02d_convex_value" % n, T.DIAG_QUADRATIC, x0, a, stop("solver"), {}))
        out.append(("diag_quadratic_n%02d_convex_first" % n, T.DIAG_QUADRATIC, x0, a, stop("solver"), dict(mode=T.FIRST)))
        a = np.concatenate([rng.uniform(0.5, 3.0, n), [1.0]])
        a[0] = -1.5            # indefinite for sure: unbounded below, ends at the iteration limit
        out.append(("diag_quadratic_n%02d_indefinite_value" % n, T.DIAG_QUADRATIC, x0, a, stop("solver", num_iterations=60),
                    {}))
    # the two scenarios of src/test/verify.cc (SOLVER_SETUP(NelderMead, RosenbrockValue)): the solver's own stop
    out.append(("scenario_verify_far", T.ROSENBROCK, np.array([[15.0, 8.0]]), None, stop("solver"), {}))
    out.append(("scenario_verify_near", T.ROSENBROCK, np.array([[-1.0, 2.0]]), None, stop("solver"), {}))
    # edges
    a = np.concatenate([rng.uniform(0.5, 3.0, 12), [0.25]])
    out.append(("edge_at_minimiser_zero", T.DIAG_QUADRATIC, np.zeros((1, 12)), a, stop("solver"), {}))   # 0.001 branch
    # (on Rosenbrock a start with equal coordinates gives equal values at the interior vertices: ties; DiagQuadratic
    # with distinct coefficients has none)
    out.append(("edge_start_1e-7", T.DIAG_QUADRATIC, np.full((1, 12), 1e-7), a, stop("solver"), {}))     # below `> 1e-6`
    out.append(("edge_start_1e-6", T.DIAG_QUADRATIC, np.full((1, 12), 1e-6), a, stop("solver"), {}))     # on it: 0.001
    out.append(("edge_start_2e-6", T.DIAG_QUADRATIC, np.full((1, 12), 2e-6), a, stop("solver"), {}))     # above: 0.05 |x|
    # small starts: the initial perturbations 0.05 |x_r| are at most 0.02, so the simplex soon lies within 1e-2 of its best
    out.append(("edge_restart", T.ROSENBROCK, rng.uniform(-0.4, 0.4, (8, 7)), None, stop("solver"),
                dict(degenerate_tol=1e-2)))
    # gamma = 1: the inside contraction point IS the worst vertex, `f_c < f[worst]` fails, the simplex shrinks
    out.append(("edge_certain_shrink", T.ROSENBROCK, rng.uniform(-2.0, 2.0, (8, 7)), None, stop("solver"),
                dict(gamma=1.0, sigma=0.25)))
    out.append(("edge_x_delta_violations_1", T.ROSENBROCK, rng.uniform(-2.0, 2.0, (8, 3)), None,
                stop("solver", x_delta_violations=1, x_delta=1e-4), {}))
    out.append(("edge_x_delta_violations_5", T.ROSENBROCK, rng.uniform(-2.0, 2.0, (8, 3)), None,
                stop("solver", x_delta_violations=5, x_delta=1e-4), {}))
    return out


def main():
    with tempfile.TemporaryDirectory() as d:
        ref = T.reference_solver(T.build_reference(d))
        arrays = {}
        for name, obj, x0, params, st, cfg in cases():
            st, c = T.make_stop(**st), T.make_config(**cfg)
            assert 0 < int(st["num_iterations"][0]) <= CAP
            x, f, g, p = ref(obj, x0, params, st, c)
            # the cap on ties, from the project's own twin in reference order
            tied = T.twin_solve(obj, x0, params, st, c, order=T.REF_ORDER)[4]
            ok = nm_cases.comparable(tied, x, f)
            print("%-40s status %s  it %s  tied %d  compared %d" % (name, sorted(set(p["status"].tolist())),
                                                                     (p["num_iterations"].min(), p["num_iterations"].max()),
                                                                     tied.sum(), ok.sum()))
            rec = dict(objective=np.int32(obj), x0=x0, params=params if params is not None else np.zeros(1),
                       stop=st, config=c, x=x, f=f, g=g, progress=p)
            if x0.shape[0] == 1:
                # single-start cases: the states the reference's step callback sees after every Progress::Update —
                # trajectory rows (num_iterations, status, value, x_delta, f_delta, gradient_norm) and the iterates
                tx, tf, tg, tp, rows, xs = ref(obj, x0, params, st, c, trajectory=CAP + 1)
                assert tx.tobytes() == x.tobytes() and len(rows) == int(p["num_iterations"][0])
                rec.update(trajectory=rows, trajectory_x=xs)
            for k, v in rec.items():
                arrays[name + "/" + k] = v
        np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
