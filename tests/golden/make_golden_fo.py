"""Writes tests/golden/first_order_reference_vectors.npz: GradientDescent and ConjugatedGradientDescent solves of the
reference (its solver/gradient_descent.h, solver/conjugated_gradient_descent.h and the two line-search headers over the
Eigen stand-in, tests/first_order/ref_harness.cpp compiled into a temporary directory outside the tree).  Run by hand
where the reference tree exists, after build():
    python tests/golden/make_golden_fo.py

Every case is a dict of arrays: method, objective, x0 (or x0_q, see fo_cases.py), params, stop, config, marked and the
reference's f, progress (status, num_iterations, nfev, x_delta, f_delta, gradient_norm; the trial points are not
observable from outside it) and x, g — in full up to n = 33, as SHA-256 digests of their bytes above (fo_cases.py says
why); single-start cases also hold the states the reference's step callback sees.  Every solve caps num_iterations at
CAP.  The assertions at the end come from counters the twin returns: if one fails, change the starts or the cap, not the
assertion."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fo_cases  # noqa: E402
import fo_lib as T  # noqa: E402

OUT = os.path.join(HERE, "first_order_reference_vectors.npz")
CAP = int(os.environ.get("FO_GOLDEN_CAP", "60"))
CEILING = 300
ND_GOLDEN = os.path.join(HERE, "newton_descent_reference_vectors.npz")
CONSERVATIVE = dict(gradient_norm=5e-6, past=5, past_delta=1e-10)   # progress.h:456-464


def stop(preset, **kw):
    return {**T.STOP_PRESETS[preset], "num_iterations": CAP, **kw}


def quantised_starts(rng, n, B, scales):
    """x0 = 1 + s k / 128 with k an integer in [-128, 128] and s drawn per row from `scales`: (k, s), see
    fo_cases.starts_from"""
    return rng.integers(-128, 129, size=(B, n)).astype(np.int16), rng.choice(scales, size=B)


def cases():
    """(name, objective, x0 or (k, s), params, {method: stop dict})"""
    rng = np.random.default_rng(20261019)
    GD, CG = T.GRADIENT_DESCENT, T.CONJUGATED_GRADIENT_DESCENT
    both = lambda st: {GD: st, CG: st}   # noqa: E731
    out = []
    # the scenarios of src/test/verify.cc: SOLVER_SETUP_CONSERVATIVE(GradientDescent, RosenbrockGradient) and
    # SOLVER_SETUP(ConjugatedGradientDescent, RosenbrockGradient), here under the cap
    scen = {GD: stop("default", **CONSERVATIVE), CG: stop("default")}
    out.append(("scenario_verify_far", T.ROSENBROCK, np.array([[15.0, 8.0]]), None, scen))
    out.append(("scenario_verify_near", T.ROSENBROCK, np.array([[-1.0, 2.0]]), None, scen))
    for n in (2, 7, 8, 9, 32, 33, 64, 65, 128, 200, 256):
        x0 = quantised_starts(rng, n, 8, (0.01, 0.1) if n <= 9 else (0.001, 0.01))
        for preset in ("default", "parity"):
            out.append(("rosenbrock_n%03d_%s" % (n, preset), T.ROSENBROCK, x0, None, both(stop(preset))))
    for n in (5, 32, 100):
        a = np.concatenate([rng.uniform(0.5, 3.0, n), [0.25]])
        out.append(("diag_quadratic_n%03d" % n, T.DIAG_QUADRATIC, rng.uniform(-2.0, 2.0, (8, n)), a,
                    both(stop("default"))))
    out.append(("quartic_n01", T.QUARTIC, rng.uniform(-3.0, 3.0, (8, 1)), None, both(stop("default"))))
    out.append(("quartic_n03", T.QUARTIC, rng.uniform(-3.0, 3.0, (8, 3)), None, both(stop("default"))))
    out.append(("quartic_single", T.QUARTIC, np.array([[0.1]]), None, both(stop("default", gradient_norm=1e-10))))
    out.append(("rosenbrock_single", T.ROSENBROCK, np.array([[-1.2, 1.0, 0.8, 1.1, 0.9]]), None, both(stop("parity"))))
    out.append(("edge_at_minimiser", T.ROSENBROCK, np.ones((2, 7)), None, both(stop("default"))))
    out.append(("edge_overflow", T.ROSENBROCK, np.full((2, 4), 1e100), None, both(stop("default"))))
    # g = 2 a x around 1e-170: g.g underflows to 0 and More-Thuente refuses the search; ConjugatedGradientDescent divides
    # by it at the second step
    a = np.array([1.0, 2.0, 0.5, 0.0])
    out.append(("edge_gg_underflow", T.DIAG_QUADRATIC, np.array([[1e-170, -2e-171, 3e-172], [0.0, 1e-200, 0.0]]), a,
                both(stop("default", gradient_norm=0.0, x_delta=0.0, num_iterations=3))))
    return out


def main():
    assert CAP <= CEILING
    with tempfile.TemporaryDirectory() as d:
        lib = T.build_reference(d)
        ref = T.reference_solver(lib)
        arrays, marked_names, names = {}, [], []
        tot = {m: dict(alpha_one=0, alpha_less=0, alpha_min=0, refused=0, max_trials=0, max_it=0) for m in (0, 1)}
        for base, obj, x0, params, stops in cases():
            for method in (T.GRADIENT_DESCENT, T.CONJUGATED_GRADIENT_DESCENT):
                name = T.METHOD_NAMES[method] + "_" + base
                st, c = T.make_stop(**stops[method]), T.make_config()
                assert 0 < int(st["num_iterations"][0]) <= CEILING
                rec = dict(method=np.int32(method), objective=np.int32(obj),
                           params=params if params is not None else np.zeros(1), stop=st, config=c)
                if isinstance(x0, tuple):
                    rec.update(x0_q=x0[0], x0_scale=x0[1])
                    x0v = fo_cases.starts_from(x0[0], x0[1])
                else:
                    rec.update(x0=x0)
                    x0v = x0
                twin = T.twin_solve(method, obj, x0v, params, st, c, order=T.REF_ORDER, counters=True)
                cnt = twin[4]
                dev = T.twin_solve(method, obj, x0v, params, st, c, order=T.DEVICE_ORDER)
                marked = bool(fo_cases.misses_contract(twin, dev).any())
                x, f, g, p = ref(method, obj, x0v, params, st, c)
                t = tot[method]
                t["alpha_one"] += int(cnt["alpha_one_steps"].sum())
                t["alpha_less"] += int(cnt["alpha_less_steps"].sum())
                t["alpha_min"] += int(cnt["alpha_min_exits"].sum())
                t["refused"] += int(cnt["refused_searches"].sum())
                t["max_trials"] = max(t["max_trials"], int(cnt["max_trials"].max()))
                t["max_it"] = max(t["max_it"], int(p["num_iterations"].max()))
                print("%-32s status %-10s it %-10s max trials %4d%s"
                      % (name, sorted(set(p["status"].tolist())), (p["num_iterations"].min(), p["num_iterations"].max()),
                         cnt["max_trials"].max(), "  MARKED" if marked else ""))
                names.append(name)
                if marked:
                    marked_names.append(name)
                rec.update(marked=np.int32(marked), f=f, progress=p)
                if x0v.shape[1] <= fo_cases.FULL_RECORD_MAX_N:
                    rec.update(x=x, g=g)
                else:
                    rec.update(x_sha256=fo_cases.digest(x), g_sha256=fo_cases.digest(g))
                if x0v.shape[0] == 1:
                    tx, tf, tg, tp, rows, xs = T.reference_trajectory(lib, method, obj, x0v, params, st, c,
                                                                       capacity=CEILING + 1)
                    assert tx.tobytes() == x.tobytes() and len(rows) == int(p["num_iterations"][0])
                    rec.update(trajectory=rows, trajectory_x=xs)
                for k, v in rec.items():
                    arrays[name + "/" + k] = v
        gd, cg = tot[T.GRADIENT_DESCENT], tot[T.CONJUGATED_GRADIENT_DESCENT]
        for t in (gd, cg):
            assert t["alpha_one"] >= 1 and t["alpha_less"] >= 1, "alpha = 1 and alpha < 1 must both be accepted"
        assert cg["alpha_min"] >= 1, "no Armijo search ended on alpha <= alpha_min"
        assert cg["max_it"] >= 2, "no ConjugatedGradientDescent solve reached the beta path"
        assert gd["max_trials"] >= 3, "no More-Thuente search took three trials (longest %d)" % gd["max_trials"]
        assert gd["refused"] >= 1, "no GradientDescent step took the refused-search branch"
        assert len(marked_names) <= fo_cases.MAX_MARKED_FRACTION * len(names), marked_names
        assert not [m for m in marked_names if fo_cases.never_marked(m)], marked_names
        np.savez_compressed(OUT, **fo_cases.pack(arrays))
    print("marked (%d of %d):" % (len(marked_names), len(names)), marked_names)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) <= os.path.getsize(ND_GOLDEN), "larger than the Newton-descent golden file"


if __name__ == "__main__":
    main()
