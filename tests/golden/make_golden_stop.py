"""Writes tests/golden/stopping_edge_reference_vectors.npz: the reference's solves of the stopping-edge table of
tests/stop_cases.py for TrustRegionNewton, NelderMead (value mode), NewtonDescent, GradientDescent and
ConjugatedGradientDescent, and of the non-default search constants of NewtonDescent and ConjugatedGradientDescent.  The
four ref_harness.cpp files are compiled as they stand into a temporary directory outside the tree.  Run by hand where the
reference tree exists, after build():
    python tests/golden/make_golden_stop.py

Every case is a dict of arrays: objective, x0_q / x0_scale / x0_base (stop_cases.py), params, stop, config_bytes, target
(the statuses the case is after), marked, and the reference's x, f, g, progress in full.  Every solve is capped at
stop_cases.CAP iterations.  The assertions below come from the project's twin on the CPU: if one fails, change the starts
or the thresholds in stop_cases.TUNING, not the assertion."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fo_cases  # noqa: E402
import fo_lib  # noqa: E402
import stop_cases as S  # noqa: E402

SEED = 20261102
B_EDGE, B_CONSTANTS = 6, 8
DIAG_EDGE, SPILL_EDGE = "x_delta_needs_3", "f_delta_abs"
FAR_SCALES = {"f_delta_rel": "f_rel_scales", "grad_abs": "grad_abs_scales"}


def quantised(rng, n, B, scales):
    return rng.integers(-128, 129, size=(B, n)).astype(np.int16), rng.choice(scales, size=B)


def cases(key):
    """(name, edge or None, objective, (k, s, base), params, stop, config, target) of one solver"""
    sv = S.SOLVERS[key]
    rng = np.random.default_rng(SEED)
    far = np.random.default_rng(SEED + 1)       # the flag edges' own starts
    scales = S.TUNING[key]["scales"]
    table = S.edges(key)
    out = []
    q = quantised(rng, 7, B_EDGE, scales) + (1.0,)
    for edge in S.EDGE_NAMES:
        over, target = table[edge]
        qe = quantised(far, 7, B_EDGE, S.TUNING[key][FAR_SCALES[edge]]) + (1.0,) if edge in S.FLAG_EDGES else q
        out.append(("%s_rosenbrock_n07_%s" % (key, edge), edge, S.ROSENBROCK, qe, None, sv.make_stop(**over),
                    sv.make_config(), target))
    n = 5
    a = np.concatenate([rng.uniform(0.5, 3.0, n), [0.25]])
    # the flag edges on DiagQuadratic: f_delta_rel over a constant term of DIAG_OFFSET; grad_abs from starts up to
    # DIAG_FAR (not for Nelder-Mead, whose gradient test never fires, nor for NewtonDescent, which solves a quadratic in
    # one step)
    for edge, c0, scale in (("f_delta_rel", S.DIAG_OFFSET, S.DIAG_NEAR), ("grad_abs", 0.25, S.DIAG_FAR)):
        if edge == "grad_abs" and S.TUNING[key]["grad_abs_diag"] is None:
            continue
        over, target = S.edges(key, diag=True)[edge]
        out.append(("%s_diag_quadratic_n05_%s" % (key, edge), edge, S.DIAG_QUADRATIC,
                    quantised(far, n, B_EDGE, (scale,)) + (0.0,), np.concatenate([a[:n], [c0]]), sv.make_stop(**over),
                    sv.make_config(), target))
    over, target = table[DIAG_EDGE]
    out.append(("%s_diag_quadratic_n05_%s" % (key, DIAG_EDGE), DIAG_EDGE, S.DIAG_QUADRATIC,
                quantised(rng, n, B_EDGE, (2.0,)) + (0.0,), a, sv.make_stop(**over), sv.make_config(), target))
    n = sv.spill_n
    over, target = table[SPILL_EDGE]
    out.append(("%s_rosenbrock_n%02d_%s" % (key, n, SPILL_EDGE), SPILL_EDGE, S.ROSENBROCK,
                quantised(rng, n, B_EDGE, scales) + (1.0,), None, sv.make_stop(**over), sv.make_config(), target))
    for label, constants in S.CONSTANT_CASES.get(key, ()):
        for n in (7, 9):
            out.append(("%s_rosenbrock_n%02d_%s" % (key, n, label), None, S.ROSENBROCK,
                        quantised(rng, n, B_CONSTANTS, scales) + (1.0,), None, sv.make_stop(),
                        sv.make_config(**constants), S.NOT_THE_LIMIT))
    return out


def same_bytes(a, b):
    """(x, f, g, progress) equal byte for byte, NaNs as NaNs"""
    for u, v in zip(a[:3], b[:3]):
        if not np.array_equal(u, v, equal_nan=True):
            return False
    return all(np.array_equal(a[3][k], b[3][k], equal_nan=True) for k in S.PROGRESS_FIELDS if k != "sum_k")


def reset_taken(rows, column, threshold):
    """a below-threshold delta followed by an above-threshold one before the solve ends"""
    below = rows[:-1, column] < threshold
    above = ~(rows[:, column] < threshold)
    return any(below[i] and above[i + 1:].any() for i in range(len(below)))


def main():
    arrays, marked_names, names = {}, [], []
    flag_matters = {k: {e: 0 for e in S.FLAG_EDGES} for k in S.SOLVERS}
    strike_matters = {k: {e: 0 for e in S.ONE_STRIKE} for k in S.SOLVERS}
    resets = {"x_delta_needs_3": [], "f_delta_abs": []}
    alpha_min_exits = 0
    with tempfile.TemporaryDirectory() as d:
        libs = {}
        for key, sv in S.SOLVERS.items():
            if sv.lib not in libs:
                sub = os.path.join(d, sv.lib.__name__)
                os.mkdir(sub)
                libs[sv.lib] = sv.lib.build_reference(sub)
            ref = sv.reference(libs[sv.lib])
            for name, edge, obj, (k, s, base), params, st, c, target in cases(key):
                x0 = S.starts_from(k, s, base)
                assert int(st["num_iterations"][0]) <= S.CAP
                twin = sv.twin(obj, x0, params, st, c, order=S.REF_ORDER)
                dev = sv.twin(obj, x0, params, st, c, order=S.DEVICE_ORDER)
                if edge is None:
                    # the reference's search constants are constexpr and the harnesses do not read the config: these
                    # cases hold inputs only, and the figures printed are the reference-order twin's
                    x, f, g, p = twin
                else:
                    x, f, g, p = ref(obj, x0, params, st, c)
                    assert same_bytes((x, f, g, p), twin), name + ": the twin in reference order is not the reference"
                if key == "nm":
                    assert not sv.nm_tied(obj, x0, params, st, c).any(), name + ": a ranking met a tie"
                marked = bool(S.misses_contract(twin, dev).any())
                hit = int(np.isin(p["status"], target).sum())
                # -- what the case is for
                assert hit >= 1, name + ": no row ends in the targeted status"
                if S.ITERATION_LIMIT not in target:
                    assert (p["status"] != S.ITERATION_LIMIT).all(), name + ": a row ends on the iteration cap"
                    assert (p["num_iterations"] <= S.CAP).all(), name
                if edge in S.ONE_STRIKE and obj == S.ROSENBROCK:
                    one = st.copy()
                    for kk, vv in S.ONE_STRIKE[edge].items():
                        one[kk] = vv
                    p1 = sv.twin(obj, x0, params, one, c)[3]
                    strike_matters[key][edge] += int((p1["num_iterations"] != p["num_iterations"]).sum())
                    column, field = (3, "x_delta") if edge == "x_delta_needs_3" else (4, "f_delta")
                    for row in range(x0.shape[0]):
                        rows = sv.twin_trajectory(obj, x0[row], params, st, c)
                        if rows is not None and reset_taken(rows, column, float(st[field][0])):
                            resets[edge].append("%s row %d" % (name, row))
                flipped = ""
                if edge in S.FLAG_EDGES:
                    other = st.copy()
                    for kk, vv in S.FLAG_EDGES[edge].items():
                        assert int(st[kk][0]) != vv
                        other[kk] = vv
                    differ = int((sv.twin(obj, x0, params, other, c)[3]["num_iterations"] != p["num_iterations"]).sum())
                    flag_matters[key][edge] += differ
                    flipped = "  flag matters on %d" % differ
                if name.startswith("cg_") and name.endswith("armijo_a"):
                    cnt = fo_lib.twin_solve(sv.method, obj, x0, params, st, c, counters=True)[4]
                    alpha_min_exits += int(cnt["alpha_min_exits"].sum())
                names.append(name)
                if marked:
                    marked_names.append(name)
                print("%-40s target %-9s rows %d of %d  status %-9s it %3d..%3d%s%s" % (
                    name, list(target), hit, len(p), sorted(set(p["status"].tolist())), p["num_iterations"].min(),
                    p["num_iterations"].max(), flipped, "  MARKED" if marked else ""))
                rec = dict(objective=np.int32(obj), x0_q=k, x0_scale=s, x0_base=np.float64(base),
                           params=params if params is not None else np.zeros(1), stop=st,
                           config_bytes=c.view(np.uint8), target=np.array(target, dtype=np.int32),
                           marked=np.int32(marked))
                if edge is not None:
                    rec.update(x=x, f=f, g=g, progress=p)
                for kk, vv in rec.items():
                    arrays[name + "/" + kk] = vv
    for key, per_edge in strike_matters.items():
        for edge, count in per_edge.items():
            assert count >= 1, "%s %s: the strike count changes no row's iteration count" % (key, edge)
    print("rows whose iteration count depends on the strike count:", strike_matters)
    for key, per_edge in flag_matters.items():
        for edge, count in per_edge.items():
            if (key, edge) != ("nm", "grad_abs"):       # value mode has no gradient: the test fires under neither flag
                assert count >= 1, "%s %s: the flipped flag changes no row's iteration count" % (key, edge)
    print("rows whose iteration count depends on the flag:", flag_matters)
    for edge, where in resets.items():
        assert where, edge + ": no trajectory takes the reset branch"
        print("reset branch of %s taken by %d trajectories, e.g. %s" % (edge, len(where), where[0]))
    assert alpha_min_exits >= 1, "no Armijo search of cg armijo_a ended on alpha <= alpha_min"
    assert len(marked_names) <= S.MAX_MARKED_FRACTION * len(names), marked_names
    assert not [m for m in marked_names if S.never_marked(m)], marked_names
    np.savez_compressed(S.GOLDEN, **fo_cases.pack(arrays))
    print("marked (%d of %d):" % (len(marked_names), len(names)), marked_names)
    print("wrote", S.GOLDEN, os.path.getsize(S.GOLDEN), "bytes")
    assert os.path.getsize(S.GOLDEN) <= os.path.getsize(S.SIZE_CEILING), "larger than the first-order golden file"


if __name__ == "__main__":
    main()
