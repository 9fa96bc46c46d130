r"""GPU: tree images of the HIP engine (bbh_tree_save_fd / bbh_tree_load_fd) and `BitBirch.save` / `load` / pickle on top of
them.  Every expectation is exact: a loaded tree must be the tree that was saved - leaf for leaf, counter for counter - and
must go on like it, whatever compactions, sealed nodes and thaws lie before the save or come after the load; the CPU oracle
is the second witness.  Files with structural faults only ever meet the host check, never a kernel."""
from __future__ import annotations

import os
import pickle
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import tree_image_format as tif
from bblean_amd import BitBirch, make_fake_fingerprints
from bblean_amd._engine import HipEngine
from bblean_amd.bitbirch import fit_concurrently
from cases import MULTIROUND_CASES, make_input
from oracle_engine import OracleEngine
from test_hip_gc import _Env
from test_hip_pipe_fuzz import _rows, _same_tables
from tree_cases import case_by_name

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]


def _kw(case: dict) -> dict:
    kw = dict(branching_factor=case["bf"], threshold=case["thr"], merge_criterion=case["crit"])
    if case.get("tol") is not None:
        kw["tolerance"] = case["tol"]
    return kw


def _extra(name, n, bf, thr, crit, seed, n_features=2048, **kw):
    return dict(name=name, n=n, bf=bf, thr=thr, crit=crit, seed=seed, n_features=n_features, **kw)


# bf 3 / 50 / 254 / above 255; diameter, radius, tolerance with a table; 64, 1024 and 2048 features
ROUND_TRIP = [case_by_name(n) for n in ("diam065_3000", "radius065_1000", "toldiam03_3000", "tolradius05_1000", "bf254_4000",
                                        "f1024_1500", "f64_500", "sparse03_5000", "dups_400")]
ROUND_TRIP += [_extra("bf3_1500", 1500, 3, 0.5, "diameter", 61), _extra("bf300_9000", 9000, 300, 0.35, "diameter", 62),
               _extra("bf1000_f1024_6000", 6000, 1000, 0.4, "tolerance-diameter", 63, n_features=1024, tol=0.05)]


def _same_engine_tree(a: BitBirch, b: BitBirch, fps: np.ndarray | None = None) -> None:
    r"""`b` holds the tree `a` holds: exported leaves with their linear sums, counters, and what BitBirch makes of them."""
    ea, eb = a._engine.export_leaves(ls_width=8), b._engine.export_leaves(ls_width=8)
    for x, y, what in zip(ea, eb, ("ids", "n_samples", "centroids", "linear sums")):
        assert x.shape == y.shape and (x == y).all(), what
    assert a._engine.stats()[2:8].tolist() == b._engine.stats()[2:8].tolist()
    assert (a.get_assignments() == b.get_assignments()).all()
    assert (np.array(a.get_centroids()) == np.array(b.get_centroids())).all()
    assert a.get_cluster_mol_ids() == b.get_cluster_mol_ids()
    if fps is not None:
        assert (a.get_medoids(fps) == b.get_medoids(fps)).all()


def _image_of(path: Path) -> tuple[bytes, int]:
    r"""(file bytes, offset of the engine image): the image is the file's tail, its length the 8 bytes before it."""
    data = path.read_bytes()
    for at in range(len(data) - tif.HEADER_BYTES, 0, -1):
        if data[at:at + 8] == tif.MAGIC and int.from_bytes(data[at - 8:at], "little") == len(data) - at:
            return data, at
    raise AssertionError("no image in the file")


@pytest.mark.parametrize("case", ROUND_TRIP, ids=[c["name"] for c in ROUND_TRIP])
def test_round_trip(case, tmp_path):
    fps = make_input(case, make_fake_fingerprints)
    tree = BitBirch(**_kw(case)).fit(fps, n_features=case["n_features"])
    path = tmp_path / "tree.bbt"
    tree.save(path)
    back = BitBirch.load(path)
    _same_engine_tree(tree, back, fps)
    assert repr(back) == repr(tree) and back.num_fitted_fps == tree.num_fitted_fps
    # the image carries no pool capacity: at most the used part of the node pools, the used cluster features and the
    # fixed part (the 512-byte header and the tolerance table)
    data, at = _image_of(path)
    h = tif.parse_header(data[at:at + tif.HEADER_BYTES])
    F = h["F"]
    used_cf = h["n8"] * F + h["n16"] * F * 2 + h["n32"] * F * 4
    assert h["image_bytes"] == len(data) - at
    assert h["image_bytes"] <= int(tree._engine.memory()[1]) + used_cf + tif.HEADER_BYTES + h["tol_bytes"]
    assert h["tol_len"] == (1001 if case["crit"].startswith("tolerance-") and case["crit"] != "tolerance-legacy" else 0)
    assert int(back._engine.memory()[1]) <= int(tree._engine.memory()[1])


def test_round_trip_mixed_width_buffers(tmp_path):
    r"""A tree that received `_fit_buffers` tables of mixed widths: cf16 and cf32 hold leaf BitFeatures."""
    case = case_by_name("bigclusters_6000")
    fps = make_input(case, make_fake_fingerprints)
    src = BitBirch(**_kw(case)).fit(fps)
    bufs, mols = src._bf_to_np()
    assert len(bufs) >= 2, list(bufs)
    kw = dict(branching_factor=10, threshold=0.25, merge_criterion="tolerance-diameter", tolerance=0.05)  # (bf 10: the root splits)
    tree, ora = BitBirch(**kw), BitBirch(_engine_factory=OracleEngine, **kw)
    for t in (tree, ora):
        for name in bufs:
            t._fit_buffers(np.array(bufs[name]), reinsert_index_seqs=mols[name])
    path = tmp_path / "tree.bbt"
    tree.save(path)
    data, at = _image_of(path)
    h = tif.parse_header(data[at:at + tif.HEADER_BYTES])
    assert h["n16"] > 0 and h["n32"] > 0, h
    back = BitBirch.load(path)
    _same_engine_tree(tree, back, fps)
    _same_tables(back, ora)
    # every method of the loaded object: refinement re-reads the fingerprints and re-inserts buffers
    for t in (back, ora):
        t.refine_inplace(fps, n_largest=2)
        t.recluster_inplace(iterations=1, extra_threshold=0.02)
    _same_tables(back, ora)


def _resume(rows, cut, kw, before: dict, after: dict, tmp_path):
    ora = BitBirch(_engine_factory=OracleEngine, **kw).fit(rows[:cut])
    with _Env(**before):
        one = BitBirch(**kw).fit(rows[:cut])
        src = BitBirch(**kw).fit(rows[:cut])
        mem = src._engine.memory()
        src.save(tmp_path / "a.bbt")
        assert src._engine.memory()[[0, 1, 4]].tolist() == mem[[0, 1, 4]].tolist(), "a save must not touch the pools"
    with _Env(**after):
        back = BitBirch.load(tmp_path / "a.bbt")
        for t in (ora, one, src, back):
            t.fit(rows[cut:])
    for t, what in ((one, "uninterrupted"), (src, "saved, then continued"), (back, "loaded")):
        bad = np.nonzero(t._log_leaf[-1] != ora._log_leaf[-1])[0]
        assert bad.size == 0, f"{what}: first differing element {cut + int(bad[0])}"
        assert t._engine.stats()[:7].tolist() == ora._engine.stats()[:7].tolist(), what
    _same_engine_tree(one, back)
    _same_engine_tree(src, back)
    _same_tables(back, ora)
    return src, back


_GC = dict(BBHIP_TINY_POOLS="1", BBHIP_GC_MIN_MB="0")
_PLAIN = dict(BBHIP_TINY_POOLS="0", BBHIP_GC_MIN_MB="1024")


@pytest.mark.parametrize("bf,seed,before,after", [(50, 0, _PLAIN, _PLAIN), (254, 1, _PLAIN, _PLAIN), (50, 2, _GC, _PLAIN), (254, 3, _GC, _PLAIN),
                                                  (50, 4, _GC, _GC), (254, 5, _GC, _GC), (8, 6, _GC, _GC), (50, 7, _PLAIN, _GC)])
def test_resume_equals_uninterrupted_and_oracle(bf, seed, before, after, tmp_path):
    rng = np.random.default_rng(9500 + seed)
    n = int(rng.integers(14_000, 24_000)) * (3 if bf == 254 else 1)
    rows = _rows(rng, n)
    kw = dict(branching_factor=bf, threshold=float(rng.uniform(0.25, 0.7)), merge_criterion="diameter" if seed % 3 else "tolerance-diameter", tolerance=0.05)
    src, back = _resume(rows, int(n * rng.uniform(0.35, 0.65)), kw, before, after, tmp_path)
    if before is _GC and int(src._engine.stats()[5]) >= 12:
        assert int(src._engine.memory()[4]) >= 1, "compactions were expected before the save"


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [{repo!r}, {repo!r} + "/tests"]
from bblean_amd import BitBirch
tree = BitBirch.load({path!r})
tree.fit(np.load({rows!r}))
ids, ns, cents, ls = tree._engine.export_leaves(ls_width=8)
np.savez({out!r}, leaf=tree._log_leaf[-1], ids=ids, ns=ns, cents=cents, ls=ls, stats=tree._engine.stats(), kc=tree._engine.kernel_counts(),
         assign=tree.get_assignments())
"""


@pytest.mark.parametrize("bf", [50, 254])
@pytest.mark.parametrize("switch", ["BBHIP_NO_PIPE", "BBHIP_NO_FAST"])
def test_resume_on_every_insertion_kernel(bf, switch, tmp_path):
    r"""The loaded tree (every node sealed) under the steady-state kernel alone and under the complete engine alone: the
    switches are read once per process, so the continuation runs in a child process."""
    rng = np.random.default_rng(9600 + bf)
    n = 20_000 * (3 if bf == 254 else 1)
    rows = _rows(rng, n)
    cut = n // 2
    kw = dict(branching_factor=bf, threshold=0.45, merge_criterion="diameter")
    ora = BitBirch(_engine_factory=OracleEngine, **kw).fit(rows[:cut]).fit(rows[cut:])
    BitBirch(**kw).fit(rows[:cut]).save(tmp_path / "a.bbt")
    np.save(tmp_path / "b.npy", rows[cut:])
    script = _CHILD.format(repo=str(REPO), path=str(tmp_path / "a.bbt"), rows=str(tmp_path / "b.npy"), out=str(tmp_path / "out.npz"))
    env = dict(os.environ, **{switch: "1"})
    done = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    assert (got["leaf"] == ora._log_leaf[-1]).all()
    assert got["stats"][:7].tolist() == ora._engine.stats()[:7].tolist()
    assert (got["assign"] == ora.get_assignments()).all()
    ids, ns, cents, ls = ora._engine.export_leaves(ls_width=8)
    assert (got["ids"] == ids).all() and (got["ns"] == ns).all() and (got["cents"] == cents).all() and (got["ls"] == ls).all()
    kc = got["kc"]
    assert int(kc[0]) == 0 and (switch != "BBHIP_NO_FAST" or int(kc[1]) == 0), kc.tolist()


def _many_nodes() -> tuple[BitBirch, np.ndarray]:
    r"""A tree of hundreds of nodes under an internal root: its image takes several groups."""
    fps = make_fake_fingerprints(20_000, seed=98)  # (hardly anything merges at 0.65: thousands of leaf BitFeatures)
    return BitBirch(branching_factor=50, threshold=0.65, merge_criterion="diameter").fit(fps), fps


def test_chunked_save_and_load_equal_the_default(tmp_path):
    tree, fps = _many_nodes()
    least = HipEngine.image_min_stage(2048)
    assert least == 64 * (4 * 256 + 176)
    tree.save(tmp_path / "default.bbt")
    tree.save(tmp_path / "again.bbt")
    tree.save(tmp_path / "least.bbt", stage_bytes=least)
    tree.save(tmp_path / "odd.bbt", stage_bytes=3 * least + 12345)
    ref = (tmp_path / "default.bbt").read_bytes()
    data, at = _image_of(tmp_path / "default.bbt")
    assert tif.parse_header(data[at:])["n_blocks"] > 4 * tif.GROUP_BLOCKS, "the tree must take several staging ranges"
    for name in ("again", "least", "odd"):
        assert (tmp_path / f"{name}.bbt").read_bytes() == ref, name
    with pytest.raises(RuntimeError, match="stage_bytes"):
        tree.save(tmp_path / "no.bbt", stage_bytes=least - 1)
    with pytest.raises(RuntimeError, match="stage_bytes"):
        BitBirch.load(tmp_path / "default.bbt", stage_bytes=least - 1)
    for stage in (0, least, 2 * least):
        back = BitBirch.load(tmp_path / "default.bbt", stage_bytes=stage)
        _same_engine_tree(tree, back, fps)
        back.save(tmp_path / "back.bbt", stage_bytes=least)
        assert (tmp_path / "back.bbt").read_bytes() == ref, "a loaded tree saves to the same bytes"
    # the engine level: the image alone, at a position inside a larger file
    with open(tmp_path / "raw.bin", "w+b") as f:
        f.write(b"0123456789")
        n = tree._engine.save_image(f, stage_bytes=least)
        assert f.tell() == 10 + n
        f.write(b"tail")
        f.seek(10)
        assert HipEngine.check_image(f) == n and f.tell() == 10
        eng = HipEngine.load_image(f, stage_bytes=least)
        assert f.tell() == 10 + n and f.read() == b"tail"
    for x, y in zip(eng.export_leaves(ls_width=8), tree._engine.export_leaves(ls_width=8)):
        assert (x == y).all()
    eng.close()


def test_structural_faults_never_reach_a_kernel(tmp_path):
    tree, _ = _many_nodes()
    tree.save(tmp_path / "tree.bbt")
    data, at = _image_of(tmp_path / "tree.bbt")
    with open(tmp_path / "tree.bbt", "rb") as f:
        f.seek(at)
        assert HipEngine.check_image(f) == len(data) - at
    faults = tif.damaged(data, at)
    assert len(faults) >= 6
    for what, bad in faults.items():
        p = tmp_path / "bad.bbt"
        p.write_bytes(bad)
        with open(p, "rb") as f:
            f.seek(at)
            with pytest.raises(RuntimeError, match="tree image"):
                HipEngine.check_image(f)  # (the host check only: nothing corrupt is handed to load)


def test_two_loads_are_independent_and_fit_concurrently(tmp_path):
    rng = np.random.default_rng(9700)
    rows = _rows(rng, 30_000)
    kw = dict(branching_factor=254, threshold=0.4, merge_criterion="diameter")
    BitBirch(**kw).fit(rows[:10_000]).save(tmp_path / "a.bbt")
    t1, t2 = BitBirch.load(tmp_path / "a.bbt"), BitBirch.load(tmp_path / "a.bbt")
    fresh = BitBirch(**kw)
    fit_concurrently([t1, fresh, t2], [rows[10_000:20_000], rows[:15_000], rows[20_000:]])
    o1 = BitBirch(_engine_factory=OracleEngine, **kw).fit(rows[:10_000]).fit(rows[10_000:20_000])
    o2 = BitBirch(_engine_factory=OracleEngine, **kw).fit(rows[:10_000]).fit(rows[20_000:])
    of = BitBirch(_engine_factory=OracleEngine, **kw).fit(rows[:15_000])
    for hip, ora in ((t1, o1), (t2, o2), (fresh, of)):
        assert (hip._log_leaf[-1] == ora._log_leaf[-1]).all()
        _same_tables(hip, ora)


def test_unfitted_and_reset_trees(tmp_path):
    tree = BitBirch(branching_factor=254, threshold=0.5, merge_criterion="tolerance-radius", tolerance=0.1)
    tree.save(tmp_path / "new.bbt")
    back = BitBirch.load(tmp_path / "new.bbt")
    assert not back.is_init and back._engine is None and back.tolerance == 0.1
    fps = make_fake_fingerprints(3000, seed=11)
    tree.fit(fps)
    tree.reset()  # an engine with pools and an empty root
    tree.save(tmp_path / "reset.bbt")
    back = BitBirch.load(tmp_path / "reset.bbt")
    ora = BitBirch(branching_factor=254, threshold=0.5, merge_criterion="tolerance-radius", tolerance=0.1, _engine_factory=OracleEngine)
    back.fit(fps)
    ora.fit(fps)
    _same_tables(back, ora)
    # an engine that never received anything: an image without nodes
    eng = HipEngine(50, 0.65, 0, 0.0, np.zeros(0), 2048)
    with open(tmp_path / "empty.bin", "w+b") as f:
        n = eng.save_image(f)
        assert n == tif.HEADER_BYTES
        f.seek(0)
        twin = HipEngine.load_image(f)
    assert twin.leaf_count() == 0 and (twin.fit_packed(fps[:500]) == eng.fit_packed(fps[:500])).all()


def test_estimators_pickle():
    import torch

    from bblean_amd.sklearn import BitBirch as SkBitBirch, UnpackedBitBirch

    fps = make_fake_fingerprints(3000, seed=21)
    qry = make_fake_fingerprints(700, seed=22)
    for cls, unpacked in ((SkBitBirch, False), (UnpackedBitBirch, True)):
        assert pickle.loads(pickle.dumps(cls(threshold=0.4))).get_params() == cls(threshold=0.4).get_params()
        est = cls(threshold=0.5, branching_factor=50)
        est.fit(np.unpackbits(fps, axis=1) if unpacked else fps)
        back = pickle.loads(pickle.dumps(est))
        assert back._packed_centers.is_cuda and (back._packed_centers == est._packed_centers).all()
        assert (back.labels_ == est.labels_).all() and (back.subcluster_centers_ == est.subcluster_centers_).all()
        q = np.unpackbits(qry, axis=1) if unpacked else qry
        assert (back.predict(q) == est.predict(q)).all()
        assert back.transform(q).tobytes() == est.transform(q).tobytes()
        tq = torch.from_numpy(qry).cuda()
        assert (back.predict(tq, input_is_packed=True) == est.predict(tq, input_is_packed=True)).all()
        a, b = back.transform(tq, input_is_packed=True), est.transform(tq, input_is_packed=True)
        a, b = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in (a, b))
        assert a.tobytes() == b.tobytes()


def test_multiround_save_tree():
    from bblean_amd.multiround import run_multiround_bitbirch

    case = MULTIROUND_CASES[0]
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        for s in case["seeds"]:
            np.save(d / f"fps.{str(s).zfill(4)}.npy", make_fake_fingerprints(case["n_per_file"], seed=s))
        (d / "out").mkdir()
        run_multiround_bitbirch(sorted(d.glob("*.npy")), d / "out", num_initial_processes=1, save_tree=True, **case["kwargs"])
        clusters = pickle.load(open(d / "out" / "clusters.pkl", "rb"))
        tree = BitBirch.load(d / "out" / "bitbirch.tree")
    assert tree.get_cluster_mol_ids() == clusters
