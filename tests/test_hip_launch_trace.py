r"""The tree launch loop decides as it did: every scenario of launch_trace_cases.py, in a fresh process with BBHIP_LAUNCH_LOG=1,
against tests/golden/launch_trace.json - recorded three times from the library of the commit named in the file
(tests/golden/make_launch_trace.py).  Per launch: engine name, tree count, element kind, criterion, elements, the six counter
deltas and the stop code (the two timing fields are dropped; a field that differed between the three recordings themselves
is listed under the scenario's "varies" and not compared); at the end bbh_tree_kernel_counts and bbh_tree_stats, for the
systolic scenarios entries 0-3 and 7 of bbh_tree_sys_counts, and the beginnings of the lines bbh_tree_stats printed."""
from __future__ import annotations

import json
import warnings
from pathlib import Path

import pytest

import launch_trace_cases as L

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "launch_trace.json").read_text())


@pytest.mark.parametrize("name", list(L.SCENARIOS))
def test_launch_trace(name):
    want = GOLDEN["scenarios"][name]
    got = L.trace(name, GOLDEN["ml_rows"])
    if name.startswith("sys_") and "level-systolic kernel: internal error" in got.get("error", ""):
        # (the opt-in kernel's own refusal to return a result, profiles/r06/sys_stability.txt: once more, as in test_hip_sys.py)
        warnings.warn(f"systolic kernel gave up: {got['error'][-300:]}")
        got = L.trace(name, GOLDEN["ml_rows"])
    assert "error" not in got, got["error"]
    keep = [k for k in L.FIELDS if k not in want["varies"]]
    launches = [[la[k] for k in keep] for la in got["launches"]]
    for i, (a, b) in enumerate(zip(launches, want["launches"])):
        assert a == b, f"launch {i}: {dict(zip(keep, a))} != recorded {dict(zip(keep, b))}"
    assert len(launches) == len(want["launches"])
    assert got["final"] == want["final"]
    assert got["reports"] == want["reports"]
    if name[len("first_stretch_"):] in ("phases", "pipe_phases", "pipe_audit"):
        assert got["reports"], "bbh_tree_stats printed no report"


def test_sys_is_not_taken_without_out_leaf():
    r"""BBHIP_SYS=1, through the raw ABI: a fit with out_leaf = NULL does not go to the systolic kernel (its BitFeature ids could not
    be renumbered into insertion order), one with an out_leaf does; both trees' exports equal the oracle's, field by field
    (checked in the child)."""
    done = L.child(["no_out_leaf"], {"BBHIP_SYS": "1"})
    assert done.returncode == 0, done.stderr[-3000:]
    res = json.loads(done.stdout.strip().splitlines()[-1])
    assert res["sys_launches_without_out"] == 0, res
    assert res["sys_launches_with_out"] > 0, res
