r"""Which cases of the four tree edge-case families (tree_threshold_cases, tree_split_cases, tree_storage_cases,
tree_abi_cases) the REFERENCE can express, and what is observed of them: pure data and helpers, no GPU, no reference.

Every GPU test over those families asserts libbbhip.so == oracle.  tests/golden/edges.npz (written by
tests/golden/make_golden_edges.py from runs of the reference's own BitBirch) holds what the reference makes of the cases
listed here; test_edge_reference.py holds the oracle's replay of the same cases against it, test_hip_edge_reference.py the
public bblean_amd.BitBirch on the device.

A case qualifies (`why_not`) when
  - every operation is one the reference has: ("packed", rows) -> BitBirch.fit, ("reset",) -> BitBirch.reset, or one that
    does not change what the tree holds (("compact", seal), ("reload",): the storage model's), which the reference skips;
  - its configuration is what the host's own bblean_amd.BitBirch(threshold, branching_factor, merge_criterion=name,
    tolerance=t) hands to an engine factory: found with a recording factory (`host_config`).  Branching factor, threshold,
    criterion and width must be equal; the scalar tolerance where the criterion reads it (tolerance-legacy alone does:
    tree_accept_eq in oracle/bb_oracle.c, merge_accept in bb_tree.hip); the tolerance table when both read the same value for
    every n up to the rows of the case, which no cluster can outgrow (beyond its length a table reads 0).

The observables (`leaf_observables`, `walk_observables`) are arrays; the fixture keeps their sha256 (`digests`), linear sums
hashed from a sparse form (rows x features uint64 is 400 MB for a +1-ulp ladder case).
TEST INFRASTRUCTURE - never imported by the product."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import tree_abi_cases as T
import tree_split_cases as S
import tree_storage_cases as G
import tree_threshold_cases as H
from bblean_amd._merges import CRITERION_CODES

CRITERION_NAMES = {code: name for name, code in CRITERION_CODES.items()}
HAS_TOLERANCE = ("tolerance-diameter", "tolerance-radius", "tolerance-legacy", "never-merge")
READS_SCALAR_TOLERANCE = (T.TOL_LEGACY,)
SKIPPED_OPS = ("compact", "reload")

CUSTOM_TABLE = "custom tolerance table"
BUFFERS = "BitFeature buffers"
NO_COUNTERPART = "no counterpart in the reference"
REASONS = (CUSTOM_TABLE, BUFFERS, NO_COUNTERPART)

# the groups that must keep at least one recorded case (test_edge_reference.py)
REQUIRED_GROUPS = ("ladder", "tier", "legacy", "tie", "radius", "camps", "second", "natural", "lopsided", "peel", "storage", "corners", "threshold")
GPU_MAX_ROWS = 24000


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue: id -> (group, source).  A source names a case of its family by the family's own names and tuples:
#   ("H", kind, *args)             tree_threshold_cases.build / replay_named
#   ("S", name)                    tree_split_cases.build / replay
#   ("SK", name, bf, prefixed)     tree_split_cases.kernel_case / replay_kernel
#   ("G", name)                    tree_storage_cases.build / replay
#   ("GK", bf, how, kind)          tree_storage_cases.kernel_case / replay_kernel
#   ("T", "corner", bf, F), ("T", "threshold", thr)      tree_abi_cases.corner_case, THRESHOLD_CASES / replay
# ---------------------------------------------------------------------------------------------------------------------


def _split_group(name):
    head = name.split("-")[0]
    return "camps" if head == "camps3" else "second" if head.startswith("width") else head


def _catalogue():
    rec, out = {}, []
    for case in H.SWITCH_CASES:
        if case[0] == "tol":
            out.append(("thr/" + H.case_id(case), ("H",) + case, CUSTOM_TABLE, f"tol_tables {case[3]!r}"))
        else:
            rec["thr/" + H.case_id(case)] = (case[0], ("H",) + case)
    for bf, crit, step, off, tab in H.RADIUS_CASES:
        cid = f"thr/radius-bf{bf}-crit{crit}-step{step}-{off:+d}ulp"
        if tab == "empty":
            rec[cid] = ("radius", ("H", "radius", bf, crit, step, off, tab))
        else:
            out.append((cid, ("H", "radius", bf, crit, step, off, tab), CUSTOM_TABLE, f"tol_tables {tab!r}"))
    for bf, crit, step, off in H.RADIUS_WIDE:
        cid = f"thr/radius-wide-bf{bf}-crit{crit}-step{step}-{off:+d}ulp"
        if crit == T.RADIUS:
            rec[cid] = ("radius", ("H", "radius", bf, crit, step, off, "empty", True))
        else:
            out.append((cid, ("H", "radius", bf, crit, step, off, "loose", True), CUSTOM_TABLE, "tol_tables 'loose'"))
    for bf, tab in H.TOLRAD_CASES:
        out.append((f"thr/tolrad-bf{bf}-{tab}", ("H", "tolrad", bf, tab), CUSTOM_TABLE, f"tolrad_tables {tab!r}"))
    for bf, tab in H.TOLRAD_WIDE:
        out.append((f"thr/tolrad-wide-bf{bf}-{tab}", ("H", "tolrad", bf, tab, True), CUSTOM_TABLE, f"tolrad_tables {tab!r}"))
    for crit, bf in H.BUF_CASES:
        out.append((f"thr/buffers-crit{crit}-bf{bf}", ("H", "buffers", crit, bf, 4), BUFFERS, "bbh_tree_fit_buffers at widths 1, 2, 4 and 8"))
    out.append(("thr/multi", None, NO_COUNTERPART, "MULTI_CASES: three trees in one bbh_trees_fit_packed launch; each tree alone is a recorded ladder case"))
    out.append(("thr/tiny-pools", None, NO_COUNTERPART, "TINY_CASE: BBHIP_TINY_POOLS, a pool stop and relaunch; the case alone is a recorded ladder case"))

    for name in S.CASES:
        if name.startswith("tier-"):
            out.append(("split/" + name, ("S", name), BUFFERS, "n_samples on the rows through bbh_tree_fit_buffers"))
        else:
            rec["split/" + name] = (_split_group(name), ("S", name))
    for name, bf in S.KERNEL_CASES:
        for prefixed in (False, True):
            rec[f"split-kernel/{name}-bf{bf}" + ("-prefixed" if prefixed else "")] = ("kernel-tail", ("SK", name, bf, prefixed))

    for name in G.CASES:
        if "tiers-" in name:
            out.append(("storage/" + name, ("G", name), BUFFERS, "tree_abi_cases.tier_table through bbh_tree_fit_buffers"))
        elif name == "seal_rule":
            out.append(("storage/" + name, ("G", name), NO_COUNTERPART, "a set_merge between the fits: not one of the operations replayed on the reference"))
        else:
            rec["storage/" + name] = ("storage", ("G", name))
    for case in G.KERNEL_CASES:
        rec["storage-kernel/" + G.kernel_id(case)] = ("storage", ("GK",) + case)
    out.append(("storage/multi_tree", None, NO_COUNTERPART, "three trees in one bbh_trees_fit_packed call"))

    for bf, F in T.CORNERS:
        rec[f"abi/corner-bf{bf}-F{F}"] = ("corners", ("T", "corner", bf, F))
    for thr in T.THRESHOLD_CASES:
        rec[f"abi/threshold-{thr}"] = ("threshold", ("T", "threshold", thr))
    for name in ("tol_diameter", "tol_radius"):
        out.append(("abi/" + name, ("T", "tol", name), CUSTOM_TABLE, "TOL_TABLE"))
    for name in ("tol_diameter_null", "tol_radius_null"):
        out.append(("abi/" + name, ("T", "tol", name), CUSTOM_TABLE, "tolerance 0.05 with an empty table: the host hands the exponential table"))
    out.append(("abi/merge", None, CUSTOM_TABLE, "MERGE_CFG: TOL_TABLE, then a set_merge"))
    for what in ("run tables", "tier tables", "pool table", "range tables", "switch tables", "mixed_buffers", "gather_ops"):
        out.append(("abi/" + what.replace(" ", "_"), None, BUFFERS, what + " go through bbh_tree_fit_buffers"))
    for what, why in (("strided rows", "a row stride and slabs: the rows themselves are plain packed rows"), ("misaligned rows", "base offsets and strides of the device pointer"),
                      ("mixed_packed", "several trees in one bbh_trees_fit_packed call"), ("chunk_ops", "bbh_tree_gather_buffers in chunks of 2^22 positions"),
                      ("position_sets", "bbh_tree_gather_buffers")):
        out.append(("abi/" + what.replace(" ", "_"), None, NO_COUNTERPART, why))
    return rec, out


RECORDED, LEFT_OUT = _catalogue()


def build_source(src):
    r"""-> (cfg, ops) of a source."""
    if src[0] == "H":
        return H.build(*src[1:])
    if src[0] == "S":
        return S.build(src[1])
    if src[0] == "SK":
        return S.kernel_case(*src[1:])
    if src[0] == "G":
        return G.build(src[1])[:2]
    if src[0] == "GK":
        return G.kernel_case(*src[1:])
    assert src[0] == "T"
    if src[1] == "corner":
        c, rows = T.corner_case(*src[2:])
        return c, [("packed", rows)]
    if src[1] == "threshold":
        return T.THRESHOLD_CASES[src[2]], [("packed", T.threshold_rows())]
    assert src[1] == "tol"
    return T.tol_cases()[src[2]], [("packed", T.tol_rows())]


def build(cid):
    return build_source(RECORDED[cid][1])


def n_rows(ops):
    return sum(op[1].shape[0] for op in ops if op[0] in ("packed", "buffers"))


# ---------------------------------------------------------------------------------------------------------------------
# does the reference have this case
# ---------------------------------------------------------------------------------------------------------------------


def public_kwargs(c):
    r"""The constructor arguments, of the reference's BitBirch and of bblean_amd's alike, that stand for a raw configuration."""
    name = CRITERION_NAMES[int(c["crit"])]
    kw = dict(threshold=c["thr"], branching_factor=c["bf"], merge_criterion=name)
    if name in HAS_TOLERANCE:
        kw["tolerance"] = c["tol"]
    return kw


class _Recorder:
    r"""An engine factory that only writes down what bblean_amd.BitBirch hands it."""

    def __init__(self, branching_factor, threshold, criterion, tolerance, tol_table, n_features, device=0):
        self.got = dict(bf=branching_factor, thr=threshold, crit=criterion, tol=tolerance, table=np.array(tol_table, dtype=np.float64), F=n_features)

    def fit_packed(self, rows, stream=None):
        return np.zeros(len(rows), np.uint32)


def host_config(c):
    r"""What bblean_amd.BitBirch(**public_kwargs(c)) hands to its engine factory for a tree of c["F"] features."""
    from bblean_amd import BitBirch

    tree = BitBirch(_engine_factory=_Recorder, **public_kwargs(c))
    tree.fit(np.zeros((1, c["F"] // 8), np.uint8))
    return tree._engine.got


def table_reads(table, n):
    r"""What a criterion reads from a tolerance table for clusters of 0 .. n members: 0 beyond its end."""
    out = np.zeros(n + 1, np.float64)
    k = min(len(table), n + 1)
    out[:k] = np.asarray(table, np.float64)[:k]
    return out


def why_not(c, ops):
    r"""-> None when the reference can express the case, else one of REASONS."""
    kinds = {op[0] for op in ops}
    if "buffers" in kinds:
        return BUFFERS
    if kinds - {"packed", "reset"} - set(SKIPPED_OPS):
        return NO_COUNTERPART
    host = host_config(c)
    same = [host[k] == c[k] for k in ("bf", "thr", "crit", "F")]
    assert all(same), ("the host hands another configuration", host, c)
    n = n_rows(ops)
    if not (table_reads(host["table"], n) == table_reads(c["table"], n)).all():
        return CUSTOM_TABLE
    if int(c["crit"]) in READS_SCALAR_TOLERANCE:
        assert host["tol"] == c["tol"], (host["tol"], c["tol"])
    return None


def calls(ops):
    r"""-> the calls of the public class for a list of operations: ("fit", rows) and ("reset",)."""
    out = []
    for op in ops:
        if op[0] == "packed":
            out.append(("fit", op[1]))
        elif op[0] == "reset":
            out.append(("reset",))
        else:
            assert op[0] in SKIPPED_OPS, op[0]
    return out


def input_digest(ops):
    h = hashlib.sha256()
    for call in calls(ops):
        h.update(call[0].encode())
        if call[0] == "fit":
            rows = np.ascontiguousarray(call[1], dtype=np.uint8)
            h.update(np.array(rows.shape, np.int64).tobytes())
            h.update(rows.tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# observables.  Linear sums are (counts, cols, vals): per row the number of non-zero features, then all their columns and
# values row after row.
# ---------------------------------------------------------------------------------------------------------------------


def sparse_rows(ls, chunk=512):
    r"""Dense (rows, F) -> (counts, cols, vals), a few rows at a time."""
    counts, cols, vals = [], [], []
    for lo in range(0, ls.shape[0], chunk):
        part = np.asarray(ls[lo:lo + chunk])
        r, c = np.nonzero(part)
        counts.append(np.bincount(r, minlength=part.shape[0]))
        cols.append(c)
        vals.append(part[r, c])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return cat(counts, np.uint32), cat(cols, np.uint32), cat(vals, np.uint64)


def sparse_of_snapshot(snap):
    r"""The leaves' linear sums of a tree_abi_cases.snapshot (dense `ls`) or of its tree_threshold_cases.compact form."""
    if "ls" in snap:
        return sparse_rows(snap["ls"])
    rows, F = (int(v) for v in snap["ls_shape"])
    nz = snap["ls_nz"].astype(np.int64)
    return np.bincount(nz // F, minlength=rows).astype(np.uint32), (nz % F).astype(np.uint32), snap["ls_val"].astype(np.uint64)


def leaf_observables(ops, snap):
    r"""What the public class shows of a tree, worked out from a raw snapshot (tree_abi_cases.snapshot with the out_leaf of
    every fit) as bblean_amd.BitBirch works it out: the cluster count after every fit call (a leaf BitFeature never goes
    away, so it is the number of BitFeatures the elements so far ended in), the members of every BitFeature in chain order and
    insertion order (get_cluster_mol_ids(sort=False)), the labels 1 .. K by size, stable (get_assignments), the centroids
    in chain order (get_centroids(sort=False)), n_samples and linear sums of the leaves."""
    outs = list(snap["out_leaf"])
    assert len(outs) == sum(op[0] == "packed" for op in ops)
    counts, cur = [], []
    for op in ops:
        if op[0] == "packed":
            cur.append(np.asarray(outs.pop(0), np.int64))
            counts.append(len(np.unique(np.concatenate(cur))))
        elif op[0] == "reset":
            cur = []
    elem = np.concatenate(cur) if cur else np.zeros(0, np.int64)
    ids, ns = np.asarray(snap["ids"], np.int64), np.asarray(snap["ns"], np.int64)
    pos = np.full(int(max(ids.max(initial=0), elem.max(initial=0))) + 1, -1, np.int64)
    pos[ids] = np.arange(ids.size)
    chain = pos[elem]
    assert (chain >= 0).all() and (np.bincount(chain, minlength=ids.size) == ns).all(), "out_leaf and the exported leaves disagree"
    label = np.empty(ids.size, np.int64)
    label[np.argsort(-ns, kind="stable")] = np.arange(1, ids.size + 1)
    return dict(counts=np.array(counts, np.int64), assign=label[chain].astype(np.uint32), members=np.argsort(chain, kind="stable").astype(np.uint32),
                ns=ns.astype(np.uint64), cents=np.ascontiguousarray(snap["cents"], dtype=np.uint8), ls=sparse_of_snapshot(snap))


def walk_observables(walk):
    r"""A pre-order walk (OracleEngine.walk, tree_image_format.Image.walk) -> nodes [depth, leaf flag, length, chain position]
    and per row n_samples, centroid and (where the walk has them) linear sum."""
    out = dict(walk_nodes=np.ascontiguousarray(walk["nodes"], dtype=np.int32), walk_n=np.asarray(walk["n"], np.uint64),
               walk_cent=np.ascontiguousarray(walk["cent"], dtype=np.uint8))
    if "ls" in walk:
        out["walk_ls"] = sparse_rows(walk["ls"])
    return out


ARRAYS = ("assign", "members", "ns", "cents", "ls", "walk_nodes", "walk_n", "walk_cent", "walk_ls")  # kept as digests
PLAIN = ("counts", "numbers")                                                                       # kept as they are


def _sha(a):
    h = hashlib.sha256()
    for part in (a if isinstance(a, tuple) else (a,)):
        part = np.ascontiguousarray(part)
        h.update(np.array(part.shape, np.int64).tobytes())
        h.update(part.tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def digests(obs):
    r"""Observables -> what the fixture keeps of them: sha256 of every array (shape and bytes), the counts per call, and
    `numbers` = [rows, clusters, nodes, walk rows, depth] (nodes, walk rows and depth only with a walk, else -1)."""
    out = {k + "_sha": _sha(obs[k]) for k in ARRAYS if k in obs}
    out["counts"] = np.asarray(obs["counts"], np.int64)
    walk = "walk_nodes" in obs
    out["numbers"] = np.array([obs["assign"].size, obs["ns"].size, len(obs["walk_nodes"]) if walk else -1, obs["walk_n"].size if walk else -1,
                               int(obs["walk_nodes"][:, 0].max(initial=0)) if walk else -1], np.int64)
    return out


def first_difference(got, want):
    r"""Two sets of observables -> the lines that say where they differ first, observable by observable (empty: they are
    equal in all that both hold)."""
    lines = []
    for k in ("counts",) + ARRAYS:
        if k not in got or k not in want:
            continue
        a, b = got[k], want[k]
        if isinstance(a, tuple):  # sparse linear sums: find the row
            (ca, xa, va), (cb, xb, vb) = a, b
            if ca.shape != cb.shape:
                lines.append(f"{k}: {ca.size} rows against {cb.size}")
            sa, sb = (np.concatenate([[0], np.cumsum(x.astype(np.int64))]) for x in (ca, cb))
            for r in range(min(ca.size, cb.size)):
                ra = (xa[sa[r]:sa[r + 1]], va[sa[r]:sa[r + 1]])
                rb = (xb[sb[r]:sb[r + 1]], vb[sb[r]:sb[r + 1]])
                if ra[0].shape != rb[0].shape or (ra[0] != rb[0]).any() or (ra[1] != rb[1]).any():
                    da, db = dict(zip(ra[0].tolist(), ra[1].tolist())), dict(zip(rb[0].tolist(), rb[1].tolist()))
                    f = min(j for j in set(da) | set(db) if da.get(j, 0) != db.get(j, 0))
                    lines.append(f"{k}: first at row {r}, feature {f}: {da.get(f, 0)} against {db.get(f, 0)}")
                    break
            continue
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            lines.append(f"{k}: shape {a.shape} against {b.shape}")
            a, b = a[:min(len(a), len(b))], b[:min(len(a), len(b))]  # (and where the common part differs first)
        if a.shape == b.shape and (a != b).any():
            d = (a != b) if a.ndim == 1 else (a != b).any(axis=1)
            r = int(np.argmax(d))
            if a.ndim == 1 or a.shape[1] <= 8:
                what = f"{a[r].tolist()} against {b[r].tolist()}"
            else:
                j = int(np.argmax(a[r] != b[r]))
                what = f"byte {j}: {int(a[r, j])} against {int(b[r, j])}"
            lines.append(f"{k}: {int(d.sum())} of {d.size} differ, first at {r}: {what}")
    return lines


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's side: the replay of the case's own family, the one its GPU test compares libbbhip.so against
# ---------------------------------------------------------------------------------------------------------------------


def oracle_observables(cid):
    r"""The observables of the oracle's replay of a recorded case through its RAW configuration: tree_threshold_cases.replay_named,
    tree_split_cases.replay / replay_kernel, tree_storage_cases.replay / replay_kernel, tree_abi_cases.replay."""
    src = RECORDED[cid][1]
    c, ops = build_source(src)
    if src[0] == "H":
        snap = H.replay_named(*src[1:])
    elif src[0] == "S":
        snap = S.replay(src[1])[0][-1]
    elif src[0] == "SK":
        snap = S.replay_kernel(*src[1:])[0][-1]
    elif src[0] == "G":
        snap = G.replay(src[1])[-1]
    elif src[0] == "GK":
        snap = G.replay_kernel(*src[1:])[-1]
    else:
        eng = T.make_oracle(c)
        snap = T.run(eng, ops)
        snap["walk"] = eng.walk()
        eng.close()
    if "ls" not in snap and "ls_nz" not in snap:  # (the kernel replays keep the leaves' sums in the walk alone)
        import tree_image_format as IMG

        snap = dict(snap, ls=IMG.walk_leaves(snap["walk"])["ls"])
    return dict(leaf_observables(ops, snap), **walk_observables(snap["walk"]))


def public_observables(make_tree, c, ops):
    r"""The case through a public BitBirch class (make_tree(**public_kwargs(c)) -> the tree) with the fit calls of the
    generator -> (the tree, what its getters show)."""
    tree = make_tree(**public_kwargs(c))
    counts = []
    for call in calls(ops):
        if call[0] == "fit":
            tree.fit(call[1], n_features=c["F"])
            counts.append(len(tree.get_centroids(sort=False)))
        else:
            tree.reset()
    members = tree.get_cluster_mol_ids(sort=False)
    cents = tree.get_centroids(sort=False)
    return tree, dict(counts=np.array(counts, np.int64), assign=np.asarray(tree.get_assignments()).astype(np.uint32),
                      members=np.array([i for m in members for i in m], np.uint32), ns=np.array([len(m) for m in members], np.uint64),
                      cents=np.array(cents, np.uint8).reshape(len(cents), c["F"] // 8))


def against_fixture(cid, obs):
    r"""-> the fields of the fixture's record of a case that these observables do not meet (empty: all that both hold is
    equal), in words."""
    want = fixture()[cid]
    got = digests(obs)
    bad = []
    for k, v in got.items():
        if k == "numbers":
            both = (v >= 0) & (want[k] >= 0)
            if (v[both] != want[k][both]).any():
                bad.append(f"numbers [rows, clusters, nodes, walk rows, depth]: {v.tolist()} against the reference's {want[k].tolist()}")
        elif not np.array_equal(v, want[k]):
            bad.append(f"{k}: {v.tolist() if k == 'counts' else 'digest differs'}" + (f" against the reference's {want[k].tolist()}" if k == "counts" else ""))
    if "assign" in want and not np.array_equal(obs["assign"], want["assign"]):
        d = obs["assign"] != want["assign"] if obs["assign"].shape == want["assign"].shape else None
        bad.append("assign: " + (f"first at element {int(np.argmax(d))}: {obs['assign'][np.argmax(d)]} against the reference's {want['assign'][np.argmax(d)]}" if d is not None else "another length"))
    return bad


@functools.lru_cache(maxsize=None)
def fixture():
    r"""tests/golden/edges.npz as {case id: {field: array}}."""
    from pathlib import Path

    with np.load(Path(__file__).resolve().parent / "golden" / "edges.npz") as z:
        z = {k: z[k] for k in z.files}
    out = {}
    for i, cid in enumerate(str(s) for s in z["case_ids"]):
        rec = {str(f): z["sha"][i, j] for j, f in enumerate(z["sha_fields"])}
        rec["numbers"] = z["numbers"][i]
        rec["counts"] = z["counts"][z["counts_at"][i]:z["counts_at"][i + 1]]
        if z["assign_at"][i + 1] > z["assign_at"][i]:
            rec["assign"] = z["assign"][z["assign_at"][i]:z["assign_at"][i + 1]]
        out[cid] = rec
    return out


SHA_FIELDS = ("input_sha",) + tuple(k + "_sha" for k in ARRAYS)


def pack_fixture(records):
    r"""{case id: record} -> the arrays of edges.npz: one table per field over all cases (a zip member per case and field
    costs more than the 32 bytes it holds)."""
    ids = list(records)
    at = lambda key: np.concatenate([[0], np.cumsum([len(records[c].get(key, ())) for c in ids])]).astype(np.int64)  # noqa: E731
    flat = lambda key, dt: np.concatenate([np.asarray(records[c].get(key, ()), dt) for c in ids])  # noqa: E731
    return dict(case_ids=np.array(ids), sha_fields=np.array(SHA_FIELDS), sha=np.array([[records[c][f] for f in SHA_FIELDS] for c in ids], np.uint8),
                numbers=np.array([records[c]["numbers"] for c in ids], np.int64), counts=flat("counts", np.int64), counts_at=at("counts"),
                assign=flat("assign", np.uint32), assign_at=at("assign"))
