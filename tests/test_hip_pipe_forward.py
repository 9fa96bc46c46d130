r"""Parity of the pipelined insertion kernel (`k_tree_pipe`) against the CPU oracle where consecutive elements meet the same row.

The router hands the intersection of the tracking row it has just committed with the NEXT element to that element's compare
(bb_tree_pipe.inc, pipe_fwd), and the leaf engine numbers the versions of the rows it writes itself instead of reading them
back.  The tails of tests/pipe_forward_cases.py put consecutive elements on the row the element before them changed -
merged into, appended, tied with an older row - across leaf splits, launch boundaries and the end of the input, behind a
prefix that leaves the tree to the pipelined kernel.  Compared as tests/test_hip_pipe_fuzz.py does: per `fit`
call the leaf BitFeature of every element and the engine counters, at the end clusters, centroids and BitFeature tables."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pipe_forward_cases as cases
from bblean_amd import BitBirch
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu


def _same_tables(a: BitBirch, b: BitBirch) -> None:
    assert (a.get_assignments() == b.get_assignments()).all()
    assert (np.array(a.get_centroids()) == np.array(b.get_centroids())).all()
    la, lb = a._leaves(), b._leaves()
    assert (la["members"] == lb["members"]).all() and (la["n"] == lb["n"]).all()
    ba, ma = a._bf_tables(a._leaf_order(True))
    bo, mo = b._bf_tables(b._leaf_order(True))
    assert list(ba) == list(bo)
    for k in ba:
        assert (np.asarray(ba[k]) == np.asarray(bo[k])).all()
        assert (ma[k].counts == mo[k].counts).all() and (ma[k].flat == mo[k].flat).all()


def _check(tail: np.ndarray, cuts=()) -> None:
    r"""prefix + tail, cut into `fit` calls at the tail positions `cuts`: the oracle's result, element by element, and every
    tail element inserted by the pipelined kernel."""
    assert tail.shape[0] <= 3000
    rows = cases.with_prefix(tail)
    n = rows.shape[0]
    bounds = [0] + [cases.N_PREFIX + int(c) for c in cuts] + [n]
    hip, ora = BitBirch(**cases.KW), BitBirch(_engine_factory=OracleEngine, **cases.KW)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        hip.fit(rows[lo:hi])
        ora.fit(rows[lo:hi])
        bad = np.nonzero(hip._log_leaf[-1] != ora._log_leaf[-1])[0]
        assert bad.size == 0, f"first differing element {lo + int(bad[0])} of [{lo}, {hi})"
        assert hip._engine.stats()[:7].tolist() == ora._engine.stats()[:7].tolist(), (lo, hi)
    _same_tables(hip, ora)
    kc = hip._engine.kernel_counts()
    assert int(kc[:3].sum()) == n
    assert int(kc[0]) >= tail.shape[0], kc.tolist()  # (a case that ran on the steady-state kernel checks nothing here)


def test_merge_chain():
    _check(cases.merge_chain())


def test_append_then_match():
    _check(cases.append_then_match())


@pytest.mark.parametrize("older_first", [True, False])
def test_ties_keep_the_first_row(older_first):
    _check(cases.ties(older_first))


def test_other_leaf_next():
    _check(cases.other_leaf_next())


def test_across_leaf_splits_in_one_fit():
    _check(cases.split_then_duplicates())


def _first_leaf_split_in(tail: np.ndarray) -> int:
    r"""position in the tail of the first element whose insertion splits a leaf (the oracle's counter, element by element)"""
    ora = BitBirch(_engine_factory=OracleEngine, **cases.KW).fit(cases.prefix())
    before = int(ora._engine.stats()[4])
    for i in range(tail.shape[0]):
        ora.fit(tail[i:i + 1])
        if int(ora._engine.stats()[4]) != before:
            return i
    raise AssertionError("no leaf split in the tail")


@pytest.fixture(scope="module")
def split_at() -> int:
    return _first_leaf_split_in(cases.split_then_duplicates())


@pytest.mark.parametrize("delta", list(range(-6, 7)) + [64, 65, 97])
def test_across_a_launch_boundary_around_the_leaf_split(split_at, delta):
    r"""The same rows in two `fit` calls: the cut ends a launch with a forward pending (consecutive rows share their path), right
    before, at and after the element that splits the leaf, and among the near-duplicates behind it."""
    tail = cases.split_then_duplicates()
    cut = min(max(split_at + delta, 1), tail.shape[0] - 1) if delta < 64 else delta
    _check(tail, cuts=(cut,))


@pytest.mark.parametrize("n_tail", [41, 60, 90])
def test_last_element(n_tail):
    r"""The input ends on a copy of a prototype whose next copy would merge: wave 2's row loads clamp at the last row, and the
    clamped row must never be taken for element n (one merge too many in the counters, another centroid)."""
    _check(cases.merge_chain()[:n_tail])


def test_forwarded_values_are_consumed():
    r"""The phase-timer instances count the forwarded values the router's compares consumed (`#router-fwd`) and audit the waves'
    LDS state against HBM at every run end (`BBHIP_PIPE_AUDIT`; both switches are read once per process: a subprocess).
    Merge chain and append-then-match: the oracle's result, a silent audit, and the forward in use.  (The leaf engine has no
    forward and no `#leaf-fwd` counter: measured, it made the kernel slower and was taken out again - DESIGN.md section 6p.)"""
    root = Path(__file__).resolve().parent.parent
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import numpy as np\nimport pipe_forward_cases as cases\nfrom bblean_amd import BitBirch\nfrom oracle_engine import OracleEngine\n"
            "for tail in (cases.merge_chain(), cases.append_then_match()):\n"
            "    rows = cases.with_prefix(tail)\n"
            "    hip = BitBirch(**cases.KW).fit(rows)\n"
            "    ora = BitBirch(_engine_factory=OracleEngine, **cases.KW).fit(rows)\n"
            "    assert (hip._log_leaf[-1] == ora._log_leaf[-1]).all()\n"
            "    assert hip._engine.stats()[:7].tolist() == ora._engine.stats()[:7].tolist()\n"
            "    assert (np.array(hip.get_centroids()) == np.array(ora.get_centroids())).all()\n"
            "    assert int(hip._engine.kernel_counts()[0]) >= tail.shape[0]\n" % (str(root), str(root / "tests")))
    env = dict(os.environ, BBHIP_PIPE_PHASES="1", BBHIP_PIPE_AUDIT="1")
    env.pop("BBHIP_LAUNCH_LOG", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "run-end audit" not in r.stderr, r.stderr[-2000:]
    lines = [ln for ln in r.stderr.splitlines() if "[bbhip pipe phases, per insert]" in ln]
    assert len(lines) >= 2, r.stderr[-2000:]
    for ln in lines:
        m = re.search(r"#router-fwd=([0-9.]+)", ln)
        assert m is not None, ln
        assert float(m.group(1)) > 0.0, ln
