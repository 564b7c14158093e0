"""Every iterate of a device TrustRegionNewton and NewtonDescent solve against the textbook definition of the step that produced
it (tests/nstep_lib.py), on the rows of tests/nstep_cases.py: CG-Steihaug, rho, the radius and the rejection loop replayed at
200 bits; d* = -(H + safe_guard I)^-1 g from a 200-bit solve with the known alpha and both Armijo checks; the traced value and
gradient of every iterate against the definitions of tests/hp_lib.py.  The same bounds, caps and branch counts as the CPU
twins in tests/test_nstep_lib.py; nothing here is compared with a twin.

Per case one launch of the 24 problems with an amd.Trace of 8 of them, and the prefix-limited launches of those 8 for the
per-iteration nfev and sum_k, whose iterates the trace must equal bit for bit (the trace path of these kernels at every
shape).  Every row runs at the library's mapping and at lanes_per_problem = 64 (one audit where the bits agree).
"""
import os

import pytest

import nstep_cases as Nc
import nstep_lib as Ns

pytestmark = pytest.mark.gpu
LINES = []
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _lines_to_the_terminal_summary():
    yield
    import conftest
    conftest._SUMMARY_LINES.extend(LINES)


@pytest.fixture(scope="module")
def ctx(gpu_solver_factory):
    return gpu_solver_factory().ctx


@pytest.fixture(scope="module")
def dense_ctx():
    """the library built with the dense quartic example functor (objective 101)"""
    import cppnumericalsolvers_amd as amd
    user = amd.Context(0, library=os.path.join(REPO, "cppnumericalsolvers_amd", "libmi355_lbfgs_tr.so"))
    yield user
    user.close()


def _case(context, solver, row):
    import cppnumericalsolvers_amd as amd
    _, _, _, evaluate, ks = Nc.inputs(row)
    rules = Nc.rules_of(solver, row)
    cls = amd.BatchedTrustRegionNewton if solver == "trust_region" else amd.BatchedNewtonDescent
    total = Ns.Report()
    for lanes in (0, 64):
        make = lambda stop: cls(stopping_progress=stop, context=context, lanes_per_problem=lanes, **dict(row[3] or ()))

        def ran(s, lanes=lanes):
            if lanes:
                assert s.last_launch()["lanes_per_problem"] == lanes, s.last_launch()
        what = "device %s %s lanes %d" % (solver, Nc.case_id(row), lanes)
        default = lambda stop: cls(stopping_progress=stop, context=context, **dict(row[3] or ()))
        rep = Nc.audit_once(Nc.device_trajectories(make, solver, row, after_launch=ran, make_default=default if lanes else None),
                            rules, evaluate, ks, what=what)
        Nc.assert_case(rep, rules, what)
        missing = [b for b in Nc.required_branches(solver, row) if not getattr(rep, b) > 0]
        assert not missing, "%s: branches not exercised: %s (%s)" % (what, missing, rep.line())
        if lanes == 0:
            total.merge(rep)
    LINES.append("step audit, device %s %s: %s" % (solver, Nc.case_id(row), total.line()))


@pytest.mark.parametrize("row", [r for r in Nc.rows_of("trust_region") if r[0] != "dense"], ids=Nc.case_id)
def test_trust_region_steps_are_the_textbook_steps(ctx, row):
    _case(ctx, "trust_region", row)


@pytest.mark.parametrize("row", [r for r in Nc.rows_of("trust_region") if r[0] == "dense"], ids=Nc.case_id)
def test_trust_region_steps_on_the_dense_quartic(dense_ctx, row):
    """the SPD family and the indefinite one, where negative curvature ends CG on the boundary"""
    _case(dense_ctx, "trust_region", row)


@pytest.mark.parametrize("row", [r for r in Nc.rows_of("newton_descent") if r[0] != "dense"], ids=Nc.case_id)
def test_newton_descent_steps_are_the_textbook_steps(ctx, row):
    _case(ctx, "newton_descent", row)


@pytest.mark.parametrize("row", [r for r in Nc.rows_of("newton_descent") if r[0] == "dense"], ids=Nc.case_id)
def test_newton_descent_steps_on_the_dense_quartic(dense_ctx, row):
    _case(dense_ctx, "newton_descent", row)
