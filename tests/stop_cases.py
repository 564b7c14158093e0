"""The stopping-edge cases of the five solvers whose kernels call progress_stop_tests (csrc/progress_device.hpp):
TrustRegionNewton (tr), NelderMead in value mode (nm), NewtonDescent (nd), GradientDescent (gd) and
ConjugatedGradientDescent (cg).  The table (`edges`, `CONSTANT_CASES`), one front over the four twin / harness helper
modules (`SOLVERS`), and the loader of tests/golden/stopping_edge_reference_vectors.npz, which
tests/golden/make_golden_stop.py writes from the reference's own solves.

Every edge is laid over the solver's own default preset (Nelder-Mead: the conservative one with five x_delta strikes)
with num_iterations = CAP.  Starts and thresholds differ per solver so that the branch a case names actually fires
within CAP iterations: the generator asserts that from the twin, and `target` (the statuses the case is after) and
`marked` are recorded per case.  `marked` has the meaning of fo_cases.py: the twin in device order misses the 1e-6
contract against the twin in reference order on at least one row; such a case is compared with the reference on f* only,
where both converged, and with its own twin byte for byte.

Starts are stored exactly: x0 = base + s k / 128 with integer k (int16 `x0_q`), per-row s (`x0_scale`) and the scalar
`x0_base` (1 for Rosenbrock, whose minimiser is 1; 0 for DiagQuadratic).

The two edges that turn on a flag (`FLAG_EDGES`) take inputs under which the flag's scale is not 1, so that the solve
with the flag flipped is another solve: relative f_delta on Rosenbrock from far starts (f > 1 while the test is live)
and on a DiagQuadratic whose constant term is DIAG_OFFSET (fscale = 1000 throughout); the absolute gradient test with
a loose threshold from far starts, crossed while ||x||inf is well away from 1.  Nelder-Mead in value mode has no
gradient, so its gradient test never fires under either flag."""
import os

import numpy as np

import fo_cases
import fo_lib
import nd_lib
import nm_lib
import tr_lib
import tr_queue

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stopping_edge_reference_vectors.npz")
SIZE_CEILING = fo_cases.GOLDEN           # the file may not outgrow the first-order one
CAP = 300
CONTRACT = fo_cases.CONTRACT
MAX_MARKED_FRACTION = 0.25
NEVER_MARKED_EDGES = ("limit1", "everything_off_but_limit")
CONVERGED = (3, 4)
CONTINUE, ITERATION_LIMIT, X_DELTA, F_DELTA, GRADIENT = 0, 1, 2, 3, 4
NOT_THE_LIMIT = (X_DELTA, F_DELTA, GRADIENT)
ROSENBROCK, DIAG_QUADRATIC = 0, 1
REF_ORDER, DEVICE_ORDER = 0, 1
PROGRESS_FIELDS = ("status", "num_iterations", "nfev", "sum_k", "x_delta", "f_delta", "gradient_norm")
misses_contract = fo_cases.misses_contract


class Solver:
    """One front over tr_lib / nm_lib / nd_lib / fo_lib: twin(), the reference harness, the twin's trajectory."""

    def __init__(self, key, lib, preset, method=None, spill_n=9):
        self.key, self.lib, self.method, self.spill_n = key, lib, method, spill_n
        self.preset = {**lib.STOP_PRESETS[preset], "num_iterations": CAP}

    def make_stop(self, **over):
        return self.lib.make_stop(**{**self.preset, **over})

    def make_config(self, **over):
        return self.lib.make_config(**over)

    def twin(self, objective, x0, params, stop, config, order=REF_ORDER, W=None):
        """(x, f, g, progress) of the CPU twin; W: the padded width of the device order (None: the library's mapping)"""
        T = self.lib
        if T is tr_lib:
            return T.twin_solve(objective, x0, params, stop, config, 0.0, order=order, W=W)
        if T is nm_lib:
            return T.twin_solve(objective, x0, params, stop, config, order=order, W=W)[:4]
        if T is nd_lib:
            return T.twin_solve(objective, x0, params, stop, config, 0.0, order=order, W=W)
        return T.twin_solve(self.method, objective, x0, params, stop, config, order=order, width=W)

    def twin_threaded(self, objective, x0, params, stop, config, order=DEVICE_ORDER, W=None):
        """twin() of a large batch through the helper module's threaded front (Nelder-Mead's module has none)"""
        T = self.lib
        if T is tr_lib:
            return tr_queue.twin_solve(objective, x0, params, stop, config, 0.0, order=order, W=W)
        if T is nd_lib:
            return T.twin_solve_threaded(objective, x0, params, stop, config, 0.0, order=order, W=W)
        if T is fo_lib:
            return T.twin_solve_threaded(self.method, objective, x0, params, stop, config, order=order, width=W)
        return self.twin(objective, x0, params, stop, config, order, W)

    def nm_tied(self, objective, x0, params, stop, config):
        """Nelder-Mead: the rows whose ranking met two equal values (the reference's std::sort places them as it
        happens to)"""
        return self.lib.twin_solve(objective, x0, params, stop, config, order=REF_ORDER)[4]

    def twin_trajectory(self, objective, x0_row, params, stop, config, capacity=CAP + 2):
        """rows [K, 6] = num_iterations, status, value, x_delta, f_delta, gradient_norm of one start, from the twin in
        reference order; None where the twin records none (tr, nd)"""
        T = self.lib
        if T is nm_lib:
            return T.twin_solve(objective, np.asarray(x0_row).reshape(1, -1), params, stop, config, order=REF_ORDER,
                                trajectory=capacity)[5]
        if T is fo_lib:
            return T.twin_trajectory(self.method, objective, x0_row, params, stop, config, capacity=capacity)[4]
        return None

    def reference(self, lib_path):
        """solve(objective, x0, params, stop, config) -> (x, f, g, progress) of the reference harness at lib_path"""
        T = self.lib
        ref = T.reference_solver(lib_path)
        if T is fo_lib:
            return lambda objective, x0, params, stop, config: ref(self.method, objective, x0, params, stop, config)
        if T is nm_lib:
            return lambda objective, x0, params, stop, config: ref(objective, x0, params, stop, config)[:4]
        return lambda objective, x0, params, stop, config: ref(objective, x0, params, stop, config)


SOLVERS = {
    "tr": Solver("tr", tr_lib, "default", spill_n=12),
    "nm": Solver("nm", nm_lib, "solver"),
    "nd": Solver("nd", nd_lib, "default"),
    "gd": Solver("gd", fo_lib, "default", method=fo_lib.GRADIENT_DESCENT),
    "cg": Solver("cg", fo_lib, "default", method=fo_lib.CONJUGATED_GRADIENT_DESCENT),
}

# per solver: the Rosenbrock start scales (x0 = 1 + s k / 128, s drawn per row) and the thresholds of the edges.  Chosen
# on the CPU (make_golden_stop.py asserts what they are for): a second-order solver's deltas fall from 1e-2 to 1e-12 in
# three iterations, so its strike cases take loose thresholds and the gradient test off; a first-order solver creeps,
# so its starts lie close and its thresholds sit where the creep crosses them within CAP iterations.
TUNING = {
    "tr": dict(scales=(0.05, 0.5), x_delta=1e-3, f_abs=1e-6, past8=1e-4, past1=1e-3,
               f_rel=1e-2, f_rel_scales=(2.0, 4.0), f_rel_diag=1e-4,
               grad_abs=30.0, grad_abs_scales=(2.0, 4.0), grad_abs_diag=10.0,
               strike_over=dict(gradient_norm=0.0), plateau_over=dict(gradient_norm=0.0, x_delta=0.0),
               past_delta0_over={}),
    "nm": dict(scales=(0.05, 0.5), x_delta=1e-3, f_abs=1e-6, past8=1e-4, past1=1e-3,
               f_rel=1e-2, f_rel_scales=(1.0, 2.0), f_rel_diag=1e-4,
               grad_abs=1e-3, grad_abs_scales=(0.05, 0.5), grad_abs_diag=None,
               strike_over={}, plateau_over=dict(x_delta=0.0), past_delta0_over={}),
    "nd": dict(scales=(0.05, 0.5), x_delta=1e-3, f_abs=1e-6, past8=1e-4, past1=1e-3,
               f_rel=1e-2, f_rel_scales=(1.0, 2.0), f_rel_diag=1e-2,
               grad_abs=100.0, grad_abs_scales=(2.0, 4.0), grad_abs_diag=None,
               strike_over=dict(gradient_norm=0.0), plateau_over=dict(gradient_norm=0.0, x_delta=0.0),
               past_delta0_over={}),
    "gd": dict(scales=(0.01, 0.03), x_delta=1e-3, f_abs=1e-6, past8=1e-4, past1=1e-3,
               f_rel=1e-2, f_rel_scales=(2.0, 4.0), f_rel_diag=1e-4,
               grad_abs=30.0, grad_abs_scales=(2.0, 4.0), grad_abs_diag=10.0,
               strike_over={}, plateau_over={}, past_delta0_over=dict(gradient_norm=1e-2)),
    "cg": dict(scales=(0.01, 0.1), x_delta=1e-3, f_abs=1e-6, past8=1e-4, past1=1e-3,
               f_rel=1e-2, f_rel_scales=(2.0, 4.0), f_rel_diag=1e-4,
               grad_abs=10.0, grad_abs_scales=(0.5, 1.0), grad_abs_diag=10.0,
               strike_over={}, plateau_over={}, past_delta0_over={}),
}
EDGE_NAMES = ("limit_off", "everything_off_but_limit", "limit1", "x_delta_needs_3", "x_delta_violations_0",
              "f_delta_abs", "f_delta_rel", "past8", "past1", "past_delta0", "grad_abs")
# the one-strike companions of the two strike cases: solved by the twin only, to show that the count matters
ONE_STRIKE = {"x_delta_needs_3": dict(x_delta_violations=1), "f_delta_abs": dict(f_delta_violations=1)}
# the two flags: what flipping each sets.  Their Rosenbrock cases draw their own, far starts (TUNING's f_rel_scales and
# grad_abs_scales), and each has a DiagQuadratic companion: constant term DIAG_OFFSET for f_delta_rel, starts up to
# DIAG_FAR for grad_abs (grad_abs_diag None: no companion; Nelder-Mead's gradient test never fires, and NewtonDescent
# solves a quadratic in one step, after which both flags fire)
FLAG_EDGES = {"f_delta_rel": dict(f_delta_relative=0), "grad_abs": dict(gradient_norm_relative=1)}
DIAG_OFFSET, DIAG_NEAR, DIAG_FAR = 1000.0, 2.0, 32.0
TRACED_EDGES = ("x_delta_needs_3", "past8")      # one strike case and one plateau case per solver are traced on the device


def edges(key, diag=False):
    """{edge: (stop overrides, targeted statuses)} of one solver; diag: with the thresholds of the two flag edges'
    DiagQuadratic companions"""
    t = dict(TUNING[key])
    if diag:
        t.update(f_rel=t["f_rel_diag"], grad_abs=t["grad_abs_diag"])
    so = t["strike_over"]
    grad_target = NOT_THE_LIMIT if key == "nm" else (GRADIENT,)     # value mode has no gradient: the test never fires
    return {
        "limit_off": (dict(num_iterations=0), NOT_THE_LIMIT),
        "everything_off_but_limit": (dict(num_iterations=30, x_delta=0.0, gradient_norm=0.0, past=0, f_delta=0.0),
                                     (ITERATION_LIMIT,)),
        "limit1": (dict(num_iterations=1), (ITERATION_LIMIT,)),
        "x_delta_needs_3": (dict(x_delta=t["x_delta"], x_delta_violations=3, past=0, **so), (X_DELTA,)),
        "x_delta_violations_0": (dict(x_delta=t["x_delta"], x_delta_violations=0, past=0, **so), (X_DELTA,)),
        "f_delta_abs": (dict(f_delta=t["f_abs"], f_delta_violations=2, past=0, **so), (F_DELTA,)),
        "f_delta_rel": (dict(f_delta=t["f_rel"], f_delta_relative=1, f_delta_violations=1, past=0, **so), (F_DELTA,)),
        "past8": (dict(past=8, past_delta=t["past8"], **t["plateau_over"]), (F_DELTA,)),
        "past1": (dict(past=1, past_delta=t["past1"], **t["plateau_over"]), (F_DELTA,)),
        # the ring runs and can never fire
        "past_delta0": (dict(past=3, past_delta=0.0, **t["past_delta0_over"]), NOT_THE_LIMIT),
        "grad_abs": (dict(gradient_norm=t["grad_abs"], gradient_norm_relative=0, past=0), grad_target),
    }


# non-default search constants (part 4 of the issue): Rosenbrock n = 7 and 9, 8 starts
CONSTANT_CASES = {
    "cg": [("armijo_a", dict(c=1e-4, rho=0.5, alpha_min=1e-3)), ("armijo_b", dict(c=0.5, rho=0.9, alpha_min=1e-8))],
    "nd": [("armijo_a", dict(safe_guard=1e-2, armijo_c=1e-4, armijo_rho=0.5)),
           ("armijo_b", dict(safe_guard=0.0, armijo_c=0.2, armijo_rho=0.9))],
}


def starts_from(k, scale, base):
    return float(base) + scale[:, None] * (k.astype(np.float64) / 128.0)


def never_marked(name):
    return name.split("_", 1)[1].endswith(NEVER_MARKED_EDGES)


def load_cases():
    """The recorded cases: dicts of name, solver (key), objective, x0, params, stop, config, target, marked and the
    reference's x, f, g, progress."""
    arrays = fo_cases.unpack(np.load(GOLDEN), dict(stop=fo_lib.STOP_DTYPE, progress=fo_lib.PROGRESS_DTYPE))
    names = sorted({k.split("/")[0] for k in arrays})
    cases = []
    for nm in names:
        c = dict(name=nm, **{k.split("/")[1]: v for k, v in arrays.items() if k.split("/")[0] == nm})
        c["solver"] = nm.split("_", 1)[0]
        c["config"] = c.pop("config_bytes").view(SOLVERS[c["solver"]].lib.CONFIG_DTYPE)
        c["x0"] = starts_from(c["x0_q"], c["x0_scale"], c["x0_base"])
        cases.append(c)
    return cases


def twin_of(case, order, W=None):
    return SOLVERS[case["solver"]].twin(int(case["objective"]), case["x0"], case["params"], case["stop"], case["config"],
                                        order=order, W=W)


# the capped-grid re-fetch batches (tests/test_gpu_stopping_edges.py): tr_queue.mixed_rosenbrock_batch(8, 600, seed)
# under num_iterations = 40, x_delta with 3 strikes, a positive f_delta with 2 strikes and past = 8.  The thresholds are
# chosen on the CPU so that the device-order twin's results hold rows ending by x_delta, rows ending by f_delta and
# solves of many lengths: a segment then fetches its next problem with non-zero strike counters and a full ring.
CAPPED_SEED = 20261102
CAPPED_THRESHOLDS = {
    "tr": dict(x_delta=1e-3, f_delta=1e-6),
    "nm": dict(x_delta=5e-2, f_delta=1e-8),
    "nd": dict(x_delta=1e-2, f_delta=1e-6),
    "gd": dict(x_delta=1e-1, f_delta=1.0),      # loose: a first-order solve from a far start is below them at once, so
    "cg": dict(x_delta=1e-1, f_delta=1.0),      # a counter left over from the row before ends the next row early
}


def capped_stop(key):
    return SOLVERS[key].make_stop(num_iterations=40, x_delta_violations=3, f_delta_violations=2, past=8,
                                  **CAPPED_THRESHOLDS[key])
