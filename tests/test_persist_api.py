r"""CPU: `BitBirch.save` / `load` / pickle and the host-side check of tree images.

The container (JSON header, bookkeeping arrays, engine image) is exercised with a test-local engine that wraps the CPU
oracle and "images" itself by recording its inputs and replaying them on load; files that must be refused are refused by
`BitBirch.load` (ValueError naming the path) and by `bbh_tree_image_check_fd` (BBH_ERR_INVALID) without a device; the
new kernels are held to the ISA rules of tests/test_isa_medoid.py."""
from __future__ import annotations

import ctypes as C
import io
import json
import os
import pickle
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tree_image_format as tif
from bblean_amd import BitBirch, _lib, make_fake_fingerprints
from bblean_amd._merges import MergeCriterion
from oracle_engine import OracleEngine

CSRC = Path(__file__).resolve().parents[1] / "bblean_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


class ReplayEngine(OracleEngine):
    r"""The CPU oracle with `save_image` / `load_image`: the image is the list of calls that built the tree."""

    def __init__(self, *args):
        super().__init__(*args)
        a = list(args) + [0] * (7 - len(args))
        self._ctor = [int(a[0]), float(a[1]), int(a[2]), float(a[3]), int(a[5])]
        self._tab = np.ascontiguousarray(a[4], dtype=np.float64)
        self._calls: list[tuple[str, list, np.ndarray]] = []

    def set_merge(self, criterion, tolerance, tol_table, threshold, branching_factor):
        super().set_merge(criterion, tolerance, tol_table, threshold, branching_factor)
        self._calls.append(("set_merge", [int(criterion), float(tolerance), float(threshold), int(branching_factor)],
                            np.ascontiguousarray(tol_table, dtype=np.float64)))

    def reset(self):
        super().reset()
        self._calls.append(("reset", [], np.zeros(0)))

    def fit_packed(self, rows, stream=None):
        self._calls.append(("fit_packed", [], np.array(rows, dtype=np.uint8)))
        return super().fit_packed(rows, stream)

    def fit_buffers(self, bufs, stream=None):
        self._calls.append(("fit_buffers", [], np.array(bufs)))
        return super().fit_buffers(bufs, stream)

    def save_image(self, fileobj, stage_bytes=0):
        start = fileobj.tell()
        head = json.dumps({"ctor": self._ctor, "calls": [[n, a] for n, a, _ in self._calls]}).encode()
        fileobj.write(b"REPLAY01" + struct.pack("<I", len(head)) + head)
        for arr in [self._tab] + [x for _, _, x in self._calls]:
            np.lib.format.write_array(fileobj, arr, allow_pickle=False)
        return fileobj.tell() - start

    @classmethod
    def load_image(cls, fileobj, device=0):
        assert fileobj.read(8) == b"REPLAY01"
        (n,) = struct.unpack("<I", fileobj.read(4))
        head = json.loads(fileobj.read(n))
        tab = np.lib.format.read_array(fileobj, allow_pickle=False)
        bf, thr, crit, tol, nf = head["ctor"]
        self = cls(bf, thr, crit, tol, tab, nf, device)
        for name, args in head["calls"]:
            arr = np.lib.format.read_array(fileobj, allow_pickle=False)
            if name == "set_merge":
                self.set_merge(args[0], args[1], arr, args[2], args[3])
            elif name == "reset":
                self.reset()
            else:
                getattr(self, name)(arr)
        return self


def _same_tree(a: BitBirch, b: BitBirch) -> None:
    assert len(a._log_leaf) == len(b._log_leaf)
    for x, y in zip(a._log_leaf, b._log_leaf):
        assert x.dtype == y.dtype and (x == y).all()
    for x, y in zip(a._log_ids, b._log_ids):
        assert x.dtype == y.dtype and (x == y).all()
    for x, y in zip(a._log_counts, b._log_counts):
        assert (x is None) == (y is None) and (x is None or (x == y).all())
    for k in ("threshold", "branching_factor", "merge_criterion", "tolerance", "_n_features", "num_fitted_fps", "is_init",
              "_internal_released", "_n_global_clusters"):
        assert getattr(a, k) == getattr(b, k), k
    assert a.get_cluster_mol_ids() == b.get_cluster_mol_ids()
    assert a.get_cluster_mol_ids(sort=False) == b.get_cluster_mol_ids(sort=False)
    assert (a.get_assignments() == b.get_assignments()).all()
    assert (np.array(a.get_centroids()) == np.array(b.get_centroids())).all()


def _fitted(**kw) -> tuple[BitBirch, np.ndarray]:
    fps = make_fake_fingerprints(900, seed=5)
    args = dict(branching_factor=20, threshold=0.4, merge_criterion="tolerance-diameter", tolerance=0.07)
    args.update(kw)
    tree = BitBirch(_engine_factory=ReplayEngine, **args)
    tree.fit(fps[:400])
    tree.fit(fps[400:700])
    return tree, fps


def test_container_round_trip_fit_fit_buffers_global(tmp_path):
    tree, fps = _fitted()
    other, _ = _fitted()
    bufs, mols = other._bf_to_np()
    for name in bufs:  # BitFeature buffers of mixed widths with their member lists, shifted past the fitted rows
        tree._fit_buffers(np.array(bufs[name]), reinsert_index_seqs=[[i + 700 for i in m] for m in mols[name]])
    with pytest.warns(UserWarning):
        tree.global_clustering(5, random_state=0)
    path = tmp_path / "tree.bbt"
    tree.save(path)
    back = BitBirch.load(path, _engine_factory=ReplayEngine)
    _same_tree(tree, back)
    assert (back._global_clustering_centroid_labels == tree._global_clustering_centroid_labels).all()
    assert back.get_cluster_mol_ids(global_clusters=True) == tree.get_cluster_mol_ids(global_clusters=True)
    assert (back.get_assignments(global_clusters=True) == tree.get_assignments(global_clusters=True)).all()
    # ... and both go on the same way
    tree.fit(fps[700:])
    back.fit(fps[700:])
    _same_tree(tree, back)
    assert repr(back) == repr(tree)


def test_load_hook_and_unfitted_tree(tmp_path):
    tree = BitBirch(branching_factor=33, threshold=0.55, merge_criterion="radius", _engine_factory=ReplayEngine)
    path = tmp_path / "empty.bbt"
    tree.save(path)  # never fitted: the configuration only
    back = BitBirch.load(path, _engine_loader=lambda f, dev: pytest.fail("no image expected"))
    assert (back.branching_factor, back.threshold, back.merge_criterion, back.tolerance) == (33, 0.55, "radius", None)
    assert not back.is_init and back._engine is None
    with pytest.raises(ValueError, match="not been fitted"):
        back.get_assignments()
    tree, _ = _fitted()
    tree.save(path)
    seen = []
    back = BitBirch.load(path, device=3, _engine_loader=lambda f, dev: seen.append(dev) or ReplayEngine.load_image(f, dev))
    assert seen == [3]
    _same_tree(tree, back)


def test_load_restores_the_saved_criterion_under_the_global_setter(tmp_path, monkeypatch):
    import bblean_amd.bitbirch as bbmod

    tree, _ = _fitted()
    path = tmp_path / "tree.bbt"
    tree.save(path)
    monkeypatch.setattr(bbmod, "_global_merge_accept", bbmod.get_merge_accept_fn("radius"))
    back = BitBirch.load(path, _engine_factory=ReplayEngine)
    assert back.merge_criterion == "tolerance-diameter" and back.tolerance == 0.07


def test_pickle_round_trip_of_the_tree(tmp_path):
    tree, fps = _fitted()
    for proto in (2, pickle.HIGHEST_PROTOCOL):
        back = pickle.loads(pickle.dumps(tree, protocol=proto))
        _same_tree(tree, back)
    bufs: list = []
    data = pickle.dumps(tree, protocol=5, buffer_callback=bufs.append)
    assert len(bufs) == 1 and len(data) < 2000, "the tree file travels out of band"
    back = pickle.loads(data, buffers=bufs)
    tree.fit(fps[700:])
    back.fit(fps[700:])
    _same_tree(tree, back)
    assert b"ReplayEngine" in data and pickle.loads(pickle.dumps(BitBirch(threshold=0.5))).threshold == 0.5


def test_save_refuses_a_custom_merge_criterion(tmp_path):
    class Mine(MergeCriterion):
        pass

    for crit in (Mine("diameter"), MergeCriterion("tolerance-diameter", 0.05, n_max=500)):
        tree = BitBirch(merge_criterion=crit, _engine_factory=ReplayEngine)
        tree.fit(make_fake_fingerprints(50, seed=1))
        with pytest.raises(ValueError, match="custom MergeCriterion"):
            tree.save(tmp_path / "no.bbt")
        with pytest.raises(ValueError, match="custom MergeCriterion"):
            pickle.dumps(tree)


def test_a_save_that_fails_leaves_the_target_as_it_was(tmp_path):
    good, _ = _fitted()
    path = tmp_path / "tree.bbt"
    good.save(path)
    before = path.read_bytes()
    refused = BitBirch(merge_criterion=MergeCriterion("tolerance-diameter", 0.05, n_max=500), _engine_factory=ReplayEngine)
    refused.fit(make_fake_fingerprints(50, seed=1))
    with pytest.raises(ValueError, match="custom MergeCriterion"):
        refused.save(path)
    no_image = BitBirch(_engine_factory=OracleEngine).fit(make_fake_fingerprints(50, seed=1))  # (an engine without save_image)
    with pytest.raises(ValueError, match="cannot write a tree image"):
        no_image.save(path)

    class Breaks(ReplayEngine):
        def save_image(self, fileobj, stage_bytes=0):
            fileobj.write(b"half an image")
            raise RuntimeError("the device went away")

    broken = BitBirch(_engine_factory=Breaks).fit(make_fake_fingerprints(50, seed=1))
    with pytest.raises(RuntimeError, match="went away"):
        broken.save(path)
    assert path.read_bytes() == before and sorted(p.name for p in tmp_path.iterdir()) == ["tree.bbt"]
    with pytest.raises(RuntimeError, match="went away"):
        broken.save(tmp_path / "new.bbt")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["tree.bbt"], "no partial file under the final name, no leftovers"


def test_header_and_image_must_describe_one_tree(tmp_path):
    tree, _ = _fitted()
    path = tmp_path / "tree.bbt"
    tree.save(path)
    data = path.read_bytes()
    magic_len = data.index(b"\0") + 1
    n_json = struct.unpack_from("<I", data, magic_len + 4)[0]
    header = json.loads(data[magic_len + 8:magic_len + 8 + n_json])
    header["n_features"] *= 2
    blob = json.dumps(header).encode()
    path.write_bytes(data[:magic_len] + struct.pack("<II", 1, len(blob)) + blob + data[magic_len + 8 + n_json:])
    with pytest.raises(ValueError, match=re.escape(str(path)) + ".*features"):
        BitBirch.load(path, _engine_factory=ReplayEngine)


class _BrokenLoadEngine(ReplayEngine):
    @classmethod
    def load_image(cls, fileobj, device=0):
        raise AttributeError("no such thing")


def test_an_attribute_error_while_unpickling_is_not_swallowed():
    sk = pytest.importorskip("sklearn.base")
    from bblean_amd.sklearn import BitBirch as SkBitBirch

    est = SkBitBirch(threshold=0.4, branching_factor=20)
    est._engine_factory = _BrokenLoadEngine
    est.fit(make_fake_fingerprints(100, seed=3))
    data = pickle.dumps(est)
    with pytest.raises(RuntimeError, match="no such thing"):
        pickle.loads(data)
    assert sk is not None


# ---- files that must be refused -----------------------------------------------------------------------------------
class _RawImageEngine:
    r"""Stands in for a fitted engine when a file is WRITTEN: its image is the given bytes."""

    def __init__(self, image: bytes):
        self.image = image

    def save_image(self, fileobj, stage_bytes=0):
        fileobj.write(self.image)
        return len(self.image)


def _container_with(image: bytes, path: Path) -> int:
    r"""A tree file around `image`, as `save` writes it; returns the offset of the image in the file."""
    tree = BitBirch(branching_factor=5, threshold=0.65)
    tree._engine, tree._n_features, tree._is_init, tree._num_fitted_fps = _RawImageEngine(image), 64, True, 4
    tree._log_leaf, tree._log_counts, tree._log_ids = [np.arange(4, dtype=np.uint32)], [None], [np.arange(4, dtype=np.int64)]
    tree.save(path)
    tree._engine = None
    data = path.read_bytes()
    assert data.endswith(image)
    return len(data) - len(image)


def _check_fd(data: bytes, tmp_path: Path, base: int = 0) -> tuple[int, str, int]:
    lib = _lib.load()
    p = tmp_path / "image.bin"
    p.write_bytes(data)
    n = C.c_uint64(0)
    fd = os.open(p, os.O_RDONLY)
    try:
        os.lseek(fd, base, os.SEEK_SET)
        rc = lib.bbh_tree_image_check_fd(fd, C.byref(n))
        assert os.lseek(fd, 0, os.SEEK_CUR) == base, "the check leaves the offset where it was"
    finally:
        os.close(fd)
    return rc, (lib.bbh_last_error() or b"").decode(), int(n.value)


def _bad_images() -> dict[str, bytes]:
    good = tif.synthetic_image()
    im = tif.Image(bytearray(good))
    bad = {"wrong magic": b"BBHTREX\0" + good[8:], "wrong version": good[:8] + struct.pack("<I", 2) + good[12:],
           "big-endian mark": good[:12] + struct.pack(">I", 0x01020304) + good[16:]}
    for i, at in enumerate(im.sections):  # a cut at every section boundary (the last one is the end: one byte short) ...
        bad[f"cut at boundary {i}"] = good[:min(at, len(good) - 1)]
    for i, (a, b) in enumerate(zip([0] + im.sections[:-1], im.sections)):  # ... and in the middle of every section
        if b - a > 1:
            bad[f"cut inside section {i}"] = good[:(a + b) // 2]
    h = dict(im.h)
    head = tif.pack_header(**{**h, "n32": h["n32"] + 1})
    bad["counts that do not match the section lengths"] = head + good[tif.HEADER_BYTES:]
    head = tif.pack_header(**{**h, "n_blocks": h["n_blocks"] - 1, "ctr": [h["n_blocks"] - 1] + h["ctr"][1:]})
    bad["fewer blocks than the node section holds"] = head + good[tif.HEADER_BYTES:]
    return bad


def test_host_check_accepts_the_hand_built_image_without_a_device(tmp_path):
    r"""That the check initialises no device is shown only where there is none: there the check passes and the load that
    follows fails for want of a device.  On a machine with a GPU that last part does not run and nothing here can tell
    whether the check touched the device."""
    good = tif.synthetic_image()
    rc, msg, n = _check_fd(good, tmp_path)
    assert rc == _lib.BBH_OK and n == len(good), msg
    rc, msg, n = _check_fd(b"x" * 37 + good + b"trailing", tmp_path, base=37)  # (an image inside a larger file)
    assert rc == _lib.BBH_OK and n == len(good), msg
    import torch

    if not torch.cuda.is_available():  # the check is host code: nothing above needed (or initialised) a device
        at = _container_with(good, tmp_path / "good.bbt")
        assert at > 0
        with pytest.raises(_lib.BBHipError):  # accepted by the check; only then is a device asked for
            BitBirch.load(tmp_path / "good.bbt")


@pytest.mark.parametrize("what", sorted(_bad_images()))
def test_rejected_files(what, tmp_path):
    image = _bad_images()[what]
    rc, msg, _ = _check_fd(image, tmp_path)
    assert rc == _lib.BBH_ERR_INVALID and msg, (what, rc, msg)
    path = tmp_path / "bad.bbt"
    _container_with(image, path)
    with pytest.raises(ValueError, match=re.escape(str(path))):
        BitBirch.load(path)


@pytest.mark.parametrize("what", sorted(tif.damaged(tif.synthetic_image())))
def test_structural_faults_are_refused_by_the_host_check(what, tmp_path):
    rc, msg, _ = _check_fd(tif.damaged(tif.synthetic_image())[what], tmp_path)
    assert rc == _lib.BBH_ERR_INVALID and msg, (what, rc, msg)


def test_rejected_containers(tmp_path):
    tree, _ = _fitted()
    path = tmp_path / "tree.bbt"
    tree.save(path)
    data = path.read_bytes()
    magic_len = data.index(b"\0") + 1
    n_json = struct.unpack_from("<I", data, magic_len + 4)[0]
    cuts = [0, 4, magic_len, magic_len + 8, magic_len + 8 + n_json // 2, magic_len + 8 + n_json]
    at = cuts[-1]
    for _ in json.loads(data[magic_len + 8:at])["arrays"]:  # every array: its length word, its middle, its end
        (n,) = struct.unpack_from("<Q", data, at)
        cuts += [at + 4, at + 8, at + 8 + n // 2, at + 8 + n]
        at += 8 + n
    cuts += [at + 4, at + 8, (at + 8 + len(data)) // 2, len(data) - 1]
    bad = {f"cut at {c}": data[:c] for c in cuts}
    bad["wrong magic"] = b"XX" + data[2:]
    bad["wrong version"] = data[:magic_len] + struct.pack("<I", 99) + data[magic_len + 4:]
    bad["not a tree"] = b"\x93NUMPY" + bytes(200)
    blob = json.dumps({"format": "something else"}).encode()
    bad["another JSON"] = data[:magic_len] + struct.pack("<II", 1, len(blob)) + blob + data[cuts[5]:]
    for what, b in bad.items():
        p = tmp_path / "bad.bbt"
        p.write_bytes(b)
        with pytest.raises(ValueError, match=re.escape(str(p))):
            BitBirch.load(p, _engine_factory=ReplayEngine)


def test_sklearn_estimators_pickle_without_a_device():
    sk = pytest.importorskip("sklearn.base")
    from bblean_amd.sklearn import BitBirch as SkBitBirch, UnpackedBitBirch

    for cls in (SkBitBirch, UnpackedBitBirch):
        est = cls(threshold=0.4, branching_factor=20, merge_criterion="radius", compute_labels=False)
        back = pickle.loads(pickle.dumps(est))
        assert type(back) is cls and back.get_params() == est.get_params()
        assert sk.clone(est).get_params() == est.get_params()
    est = SkBitBirch(threshold=0.4, branching_factor=20)
    est._engine_factory = ReplayEngine
    fps = make_fake_fingerprints(300, seed=3)
    est.fit(fps)
    assert isinstance(est._packed_centers, np.ndarray)  # (the oracle has no gather_centroids: host centroids)
    back = pickle.loads(pickle.dumps(est))
    assert (back.labels_ == est.labels_).all() and (back.subcluster_centers_ == est.subcluster_centers_).all()
    assert (back._packed_centers == est._packed_centers).all()
    assert sk.clone(est).get_params() == est.get_params()


# ---- ISA guard ----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_image_kernels_isa(tmp_path):
    out = tmp_path / "bb_tree.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function",
           "--cuda-device-only", "-S", str(CSRC / "bb_tree.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = out.read_text()
    assert "bb_tree_image.inc" in (CSRC / "Makefile").read_text() and '#include "bb_tree_image.inc"' in (CSRC / "bb_tree.hip").read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S*k_img_\S+)", text, re.M)
    assert sorted(re.search(r"k_img_[a-z]+", k).group(0) for k in kernels) == ["k_img_pack", "k_img_size", "k_img_unpack"], kernels
    for name in kernels:
        start = text.index(name + ":")
        body = text[start:text.index(".Lfunc_end", start)]
        scratch = [ln.strip() for ln in body.splitlines() if ln.strip().startswith(("scratch_", "buffer_load", "buffer_store"))]
        assert not scratch, (name, scratch[:5])
        m = re.search(r"\.set " + re.escape(name) + r"\.private_seg_size, (\d+)\s*$", text, re.M)
        assert m is not None and int(m.group(1)) == 0, (name, m.group(0) if m else None)
        assert "s_swappc_b64" not in body and "s_call_b64" not in body, name
        lds = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)
        assert lds is not None and int(lds.group(1)) == 0, name
