#!/usr/bin/env python3
"""The faulty calls of tests/test_gpu_solver_refusals.py: one fault per call into the entry points of TrustRegionNewton,
NewtonDescent, NelderMead, GradientDescent and ConjugatedGradientDescent, through capi.  Every call is refused before a
kernel launch (or, for B = 0, returns MI355_OK at once).  run_all() returns {case: {"code", "message"}}, message being
the full text of mi355_lbfgs_last_error().

    python scripts/solver_refusals.py --write     # records tests/golden/solver_refusals.json

The fixture pins the wording and the codes: record it from the commit whose refusals are to be kept, and run the test on
the commit that must keep them."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "solver_refusals.json")

ONE_COORDINATE = ("trust_region_newton", "newton_descent", "nelder_mead")   # n <= 64, one coordinate per lane
FIRST_ORDER = ("gradient_descent", "conjugated_gradient_descent")          # n <= 256
HESSIAN = ("trust_region_newton", "newton_descent")
SOLVERS = ONE_COORDINATE + FIRST_ORDER


def case_list():
    """[(name, solver, fault)]: the faults of the five solvers, where the solver has that refusal."""
    out = []
    for s in SOLVERS:
        faults = ["n_above_limit", "arith_fma", "ridge_objective", "user_objective_without_kernels",
                  "user_id_not_in_library", "unknown_builtin_id", "lanes_24", "lanes_8_at_n_12"]
        faults.append("elems_2" if s in ONE_COORDINATE else "elems_2_lanes_0")
        if s in HESSIAN:
            faults.append("hessian_diagonal")
        if s in FIRST_ORDER:
            faults.append("hessian_condition_stop")
        if s == "nelder_mead":
            faults += ["mode_7", "first_mode_on_value_only_functor"]
        if s == "conjugated_gradient_descent":
            faults += ["armijo_rho_1.5", "armijo_alpha_min_0"]
        faults += ["null_x0", "empty_batch_null_pointers"]
        out += [("%s:%s" % (s, f), s, f) for f in faults]
    return out


CASES = [name for name, _, _ in case_list()]


def run_all():
    import torch
    import cppnumericalsolvers_amd as amd
    from cppnumericalsolvers_amd import _build, capi

    contexts = {}

    def context(library=None):
        if library not in contexts:
            contexts[library] = amd.Context(0, library=library and os.path.join(_build.PKG_DIR, library))
        return contexts[library]

    def config_of(solver, lib):
        if solver == "trust_region_newton":
            c = capi.TrustRegionConfig()
            capi.check(lib.mi355_trust_region_default_config(C.byref(c)))
        elif solver == "newton_descent":
            c = capi.NewtonDescentConfig()
            capi.check(lib.mi355_newton_descent_default_config(C.byref(c)))
        elif solver == "nelder_mead":
            c = capi.NelderMeadConfig()
            capi.check(lib.mi355_nelder_mead_default_config(C.byref(c)))
        elif solver == "conjugated_gradient_descent":
            c = capi.ArmijoConfig()
            capi.check(lib.mi355_armijo_default_config(C.byref(c)))
        else:
            c = None   # GradientDescent takes no config
        return c

    def one(solver, fault):
        n = 4
        if fault == "n_above_limit":
            n = 65 if solver in ONE_COORDINATE else 257
        elif fault in ("lanes_24", "lanes_8_at_n_12"):
            n = 12
        library = None
        if fault == "user_objective_without_kernels":
            library = "libmi355_lbfgs_svm.so"      # objective 100 built for Lbfgs / Lbfgsb only
        elif fault == "first_mode_on_value_only_functor":
            library = "libmi355_lbfgs_nm.so"       # objective 100: the value-only l1 functor
        ctx = context(library)
        lib = ctx._lib
        B = 2
        keep = []
        d = capi.Desc()
        d.objective, d.linesearch, d.n, d.m = capi.OBJ_ROSENBROCK, capi.LS_MORE_THUENTE, n, 1
        d.arithmetic = capi.ARITH_EXACT
        d.stop = capi.default_stop()
        config = config_of(solver, lib)

        def params(values):
            p = np.ascontiguousarray(values, dtype=np.float64)
            keep.append(p)
            d.objective_params, d.n_params = p.ctypes.data_as(C.POINTER(C.c_double)), int(p.size)

        if fault == "arith_fma":
            d.arithmetic = capi.ARITH_FMA
        elif fault == "ridge_objective":
            rows = 3
            d.objective = capi.OBJ_SQUARED_ERROR_RIDGE
            params(np.concatenate([[rows, 0.1], np.ones(rows * n)]))
            y = torch.zeros((B, rows), dtype=torch.float64, device="cuda:0")
            keep.append(y)
            d.per_problem_data, d.per_problem_stride = y.data_ptr(), rows
        elif fault == "user_objective_without_kernels":
            d.objective = capi.OBJ_USER_FIRST
            params(np.zeros(1))
        elif fault == "user_id_not_in_library":
            d.objective = capi.OBJ_USER_FIRST         # (the default library holds no user objective)
            params(np.zeros(1))
        elif fault == "unknown_builtin_id":
            d.objective = 7
        elif fault == "first_mode_on_value_only_functor":
            d.objective = capi.OBJ_USER_FIRST
            params(np.zeros(n))
            config.mode = capi.NM_MODE_FIRST
        elif fault == "lanes_24":
            d.lanes_per_problem = 24
        elif fault == "lanes_8_at_n_12":
            d.lanes_per_problem = 8
        elif fault in ("elems_2", "elems_2_lanes_0"):
            d.elems_per_lane = 2
        elif fault == "hessian_diagonal":
            h = np.ones(n)
            keep.append(h)
            d.hessian_diagonal = h.ctypes.data_as(C.POINTER(C.c_double))
        elif fault == "hessian_condition_stop":
            d.hessian_condition_stop = 1e6
        elif fault == "mode_7":
            config.mode = 7
        elif fault == "armijo_rho_1.5":
            config.rho = 1.5
        elif fault == "armijo_alpha_min_0":
            config.alpha_min = 0.0

        x0 = torch.zeros((B, n), dtype=torch.float64, device="cuda:0")
        x, g = torch.empty_like(x0), torch.empty_like(x0)
        f = torch.empty(B, dtype=torch.float64, device="cuda:0")
        progress = torch.empty(B * capi.PROGRESS_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        pointers = [x0.data_ptr(), x.data_ptr(), f.data_ptr(), g.data_ptr(), progress.data_ptr()]
        if fault == "null_x0":
            pointers[0] = None
        elif fault == "empty_batch_null_pointers":
            B, pointers = 0, [None] * 5
        entry = getattr(lib, "mi355_%s_minimize_batch" % solver)
        stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        rc = entry(ctx.handle, C.byref(d), *(() if config is None else (C.byref(config),)), B, *pointers, stream)
        torch.cuda.synchronize()
        # (the text is the failing call's; a call that succeeds leaves the thread's last text alone, so it is not recorded)
        message = (lib.mi355_lbfgs_last_error() or b"").decode() if rc != capi.MI355_OK else ""
        return {"code": int(rc), "message": message}

    try:
        return {name: one(solver, fault) for name, solver, fault in case_list()}
    finally:
        for ctx in contexts.values():
            ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--write", action="store_true", help="record tests/golden/solver_refusals.json")
    ap.add_argument("--output", default=FIXTURE)
    args = ap.parse_args()
    results = run_all()
    text = json.dumps(results, indent=1, sort_keys=True) + "\n"
    if args.write:
        os.makedirs(os.path.dirname(args.output), exist_ok=True)
        with open(args.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
