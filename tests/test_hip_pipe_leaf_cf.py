r"""Parity of the pipelined kernel's leaf engine against the CPU oracle on the branches of its cluster-feature path.

The leaf engine (bb_tree_pipe.inc, pipe_leaf; nodes of one row per lane) gets the chosen row's uint8 cluster features from its
LDS cache or from HBM, forms the dot product with one 4 x u8 dot-accumulate per dword and takes the majority vote of a merge
four bytes at a time (bb_pipe_bytes.h, walked on the host by tests/test_pipe_bytes.py); a singleton target is spread to bytes
only when the pair is accepted.  The tails of tests/pipe_leaf_cf_cases.py make the pre-compared best row stale, turn a singleton
into a pair under a pre-compare, take a BitFeature out of the uint8 tier, put every vote count on its threshold for every size
2 .. 255, and decide jobs on a full leaf.

Every case runs three ways - the phase-timer instance with the run-end audit (`BBHIP_PIPE_AUDIT`; read once per process: one
subprocess for all cases), the default instance, and pools pre-grown by next to nothing (`BBHIP_TINY_POOLS`) - and is compared
with the oracle per `fit` call (the leaf BitFeature of every element, the engine counters) and at the end (assignments,
centroids); the pipelined kernel must have inserted every element of the tail."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import pipe_forward_cases as fwd
import pipe_leaf_cf_cases as cases
from bblean_amd import BitBirch
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NAMES = sorted(cases.CASES)


def _result(tree: BitBirch) -> dict:
    return {"leaf": np.asarray(tree._log_leaf[-1]), "stats": np.asarray(tree._engine.stats()[:7]),
            "assign": np.asarray(tree.get_assignments()), "cent": np.array(tree.get_centroids())}


@pytest.fixture(scope="module")
def oracle():
    r"""the oracle's result of every case, computed once"""
    return {name: _result(BitBirch(_engine_factory=OracleEngine, **fwd.KW).fit(fwd.with_prefix(cases.CASES[name]()))) for name in NAMES}


def _same(got: dict, want: dict, n_tail: int, kc) -> None:
    bad = np.nonzero(got["leaf"] != want["leaf"])[0]
    assert bad.size == 0, f"first differing element {int(bad[0])}"
    assert got["stats"].tolist() == want["stats"].tolist()
    assert (got["assign"] == want["assign"]).all()
    assert got["cent"].shape == want["cent"].shape and (got["cent"] == want["cent"]).all()
    assert int(kc[:3].sum()) == fwd.N_PREFIX + n_tail
    assert int(kc[0]) >= n_tail, list(kc)  # (a case that ran on the steady-state kernel checks nothing here)


def _fit_here(name: str):
    tail = cases.CASES[name]()
    assert tail.shape[0] <= 3000
    hip = BitBirch(**fwd.KW).fit(fwd.with_prefix(tail))
    return _result(hip), tail.shape[0], np.asarray(hip._engine.kernel_counts())


@pytest.mark.parametrize("name", NAMES)
def test_default_instance(oracle, name):
    got, n_tail, kc = _fit_here(name)
    _same(got, oracle[name], n_tail, kc)


@pytest.mark.parametrize("name", NAMES)
def test_tiny_pools(oracle, name):
    old = os.environ.get("BBHIP_TINY_POOLS")
    os.environ["BBHIP_TINY_POOLS"] = "1"
    try:
        got, n_tail, kc = _fit_here(name)
    finally:
        if old is None:
            os.environ.pop("BBHIP_TINY_POOLS", None)
        else:
            os.environ["BBHIP_TINY_POOLS"] = old
    _same(got, oracle[name], n_tail, kc)


_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import pipe_forward_cases as fwd
import pipe_leaf_cf_cases as cases
from bblean_amd import BitBirch
out = {}
for name in sorted(cases.CASES):
    print("## case", name, file=sys.stderr, flush=True)
    hip = BitBirch(**fwd.KW).fit(fwd.with_prefix(cases.CASES[name]()))
    out[name + ".leaf"] = np.asarray(hip._log_leaf[-1])
    out[name + ".stats"] = np.asarray(hip._engine.stats()[:7])
    out[name + ".assign"] = np.asarray(hip.get_assignments())
    out[name + ".cent"] = np.array(hip.get_centroids())
    out[name + ".kc"] = np.asarray(hip._engine.kernel_counts())
    sys.stderr.flush()
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def audited(tmp_path_factory):
    r"""every case in the phase-timer instance with the run-end audit: results, and the stderr lines of each case"""
    path = tmp_path_factory.mktemp("leaf_cf") / "audited.npz"
    env = dict(os.environ, BBHIP_PIPE_PHASES="1", BBHIP_PIPE_AUDIT="1")
    env.pop("BBHIP_LAUNCH_LOG", None)
    env.pop("BBHIP_TINY_POOLS", None)
    r = subprocess.run([sys.executable, "-c", _CHILD % (str(ROOT), str(ROOT / "tests")), str(path)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    log, cur = {}, None
    for ln in r.stderr.splitlines():
        if ln.startswith("## case "):
            cur = ln.split()[2]
            log[cur] = []
        elif cur is not None:
            log[cur].append(ln)
    return np.load(path), log, r.stderr


@pytest.mark.parametrize("name", NAMES)
def test_phase_timer_instance_with_audit(oracle, audited, name):
    data, log, err = audited
    assert "run-end audit" not in err, err[-2000:]
    got = {k: data[f"{name}.{k}"] for k in ("leaf", "stats", "assign", "cent")}
    _same(got, oracle[name], cases.CASES[name]().shape[0], data[f"{name}.kc"])


def _counter(lines, label: str) -> float:
    vals = [float(m.group(1)) for ln in lines if "[bbhip pipe leaf compares]" in ln
            for m in [re.search(re.escape(label) + r" ([0-9.]+)", ln)] if m]
    assert vals, lines[-5:]
    return max(vals)


def test_cases_reach_every_kind_of_job(audited):
    r"""the phase-timer instance counts the leaf engine's jobs by kind: singleton targets, uint8 cluster features from the LDS cache
    and from HBM, and the wide tier all occur, each in the case made for it"""
    _, log, _ = audited
    assert _counter(log["lazy_singleton"], "singleton target") > 0.0
    assert _counter(log["vote_boundaries"], "uint8 from the LDS cache") > 0.0
    assert _counter(log["stale_best_row"], "uint8 from HBM") > 0.0
    assert _counter(log["tier_change"], "wide tier") > 0.0
