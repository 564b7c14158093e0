"""Every iterate of a device GradientDescent and ConjugatedGradientDescent solve against the textbook definition of the step that
produced it, on the rows of tests/nstep_cases.py: the Fletcher-Reeves direction replayed at 200 bits from the traced gradients
alone with the known alpha and both Armijo checks (tests/nstep_lib.py); s a positive multiple of -g under the More-Thuente
conditions (tests/step_lib.py, Rules(solver="gradient_descent")); the traced value and gradient of every iterate against the
definitions of tests/hp_lib.py.  The same bounds, caps and branch counts as the CPU twins in tests/test_nstep_lib.py; nothing
here is compared with a twin.

Per case one launch of the 24 problems with an amd.Trace of 8 of them, and the prefix-limited launches of those 8 for the
per-iteration nfev and sum_k, whose iterates the trace must equal bit for bit.
"""
import pytest

import nstep_cases as Nc
import nstep_lib as Ns

pytestmark = pytest.mark.gpu
LINES = []
EVAL_TRIALS_ENV = "MI355_DEBUG_CG_EVAL_TRIALS"     # read when a context is created: the Armijo trials run eval, not value


@pytest.fixture(scope="module", autouse=True)
def _lines_to_the_terminal_summary():
    yield
    import conftest
    conftest._SUMMARY_LINES.extend(LINES)


@pytest.fixture(scope="module")
def ctx(gpu_solver_factory):
    return gpu_solver_factory().ctx


@pytest.fixture(scope="module")
def eval_trials_ctx():
    import cppnumericalsolvers_amd as amd
    with pytest.MonkeyPatch.context() as patch:
        patch.setenv(EVAL_TRIALS_ENV, "1")
        context = amd.Context(0)
    yield context
    context.close()


def _report(context, solver, row, W=0, E=0):
    import cppnumericalsolvers_amd as amd
    _, _, _, evaluate, ks = Nc.inputs(row)
    rules = Nc.rules_of(solver, row)
    cls = amd.BatchedGradientDescent if solver == "gradient_descent" else amd.BatchedConjugatedGradientDescent
    make = lambda stop: cls(stopping_progress=stop, context=context, lanes_per_problem=W, elems_per_lane=E)

    def ran(s):
        if W:
            ll = s.last_launch()
            assert (ll["lanes_per_problem"], ll["elems_per_lane"]) == (W, E), ll
    what = "device %s %s %dx%d" % (solver, Nc.case_id(row), W, E)
    default = lambda stop: cls(stopping_progress=stop, context=context)
    rep = Nc.audit_once(Nc.device_trajectories(make, solver, row, after_launch=ran, make_default=default if W else None),
                        rules, evaluate, ks, what=what)
    Nc.assert_case(rep, rules, what)
    missing = [b for b in Nc.required_branches(solver, row) if not getattr(rep, b) > 0]
    assert not missing, "%s: branches not exercised: %s (%s)" % (what, missing, rep.line())
    return rep


@pytest.mark.parametrize("solver", ["gradient_descent", "conjugated_gradient"])
@pytest.mark.parametrize("row", Nc.FIRST_ORDER_SHAPES, ids=Nc.case_id)
def test_first_order_steps_are_the_textbook_steps(ctx, solver, row):
    """the library's own mapping of every shape"""
    rep = _report(ctx, solver, row)
    LINES.append("step audit, device %s %s: %s" % (solver, Nc.case_id(row), rep.line()))


@pytest.mark.parametrize("solver", ["gradient_descent", "conjugated_gradient"])
@pytest.mark.parametrize("row", Nc.MAPPING_SHAPES, ids=Nc.case_id)
def test_every_built_mapping(ctx, solver, row):
    """every built (lanes, coordinates per lane) that covers n, two and four coordinates per lane among them"""
    mappings = Nc.mappings_of(row[2])
    assert mappings
    total = Ns.Report()
    for W, E in mappings:
        total.merge(_report(ctx, solver, row, W=W, E=E))
    LINES.append("step audit, device %s %s, %d mappings: %s" % (solver, Nc.case_id(row), len(mappings), total.line()))


@pytest.mark.parametrize("row", [r for r in Nc.FIRST_ORDER_SHAPES if r[2] in (7, 100)], ids=Nc.case_id)
def test_conjugated_gradient_steps_with_eval_trials(eval_trials_ctx, row):
    """the other setting of eval_trials: the trials run eval and the last trial's gradient is kept (n = 100: 64 x 2)"""
    rep = _report(eval_trials_ctx, "conjugated_gradient", row)
    LINES.append("step audit, device conjugated_gradient eval_trials %s: %s" % (Nc.case_id(row), rep.line()))
