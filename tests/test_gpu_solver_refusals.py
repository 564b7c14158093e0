"""The refusals of the five newer solvers' entry points (csrc/solver_entry.hip), pinned: every faulty call of
scripts/solver_refusals.py — one fault per call, each refused before a kernel launch — answers with the return code and
the full mi355_lbfgs_last_error() text recorded in tests/golden/solver_refusals.json (recorded from the commit before the
entry points were folded into one skeleton)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("solver_refusals", os.path.join(ROOT, "scripts", "solver_refusals.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_every_refusal_keeps_its_code_and_text():
    script = _script()
    with open(script.FIXTURE) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(script.CASES)       # the fixture holds every case of the list, and no other
    assert len(script.CASES) == 63
    got = script.run_all()
    assert sorted(got) == sorted(script.CASES)
    different = {name: (got[name], golden[name]) for name in script.CASES if got[name] != golden[name]}
    assert not different, different
    for name in script.CASES:                            # (what the list itself promises)
        empty = name.endswith(":empty_batch_null_pointers")
        assert (golden[name]["code"] == 0) == empty, name
        assert bool(golden[name]["message"]) != empty, name
