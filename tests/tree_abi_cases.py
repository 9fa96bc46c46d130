r"""Cases for the tree engine at the raw C ABI (include/bbhip.h, "Stateful tree engine"): pure data and builders, no GPU and
no library.  test_tree_abi_cases.py holds every case against the condition that makes it worth running, on the C oracle
alone; test_hip_tree_abi_edges.py replays the same cases on libbbhip.so with raw pointers and compares with ==.

A case is a tree configuration (`cfg`) and a list of operations:
    ("packed", rows)                               rows: (n, F / 8) uint8, np.packbits order
    ("buffers", table)                             table: (k, F + 1) unsigned, [linear_sum | n_samples]
    ("set_merge", crit, tolerance, tol_table, threshold, bf)
    ("reset",)
    ("compact", seal)                              bbh_tree_compact; on the oracle the storage model's compaction
    ("reload",)                                    save, bbh_tree_load_fd into a new handle, go on with that one
`replay` runs them on tests/oracle_engine.OracleEngine and returns everything observable."""
from __future__ import annotations

import numpy as np

from oracle_engine import OracleEngine

W = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
DIAMETER, RADIUS, TOL_DIAMETER, TOL_RADIUS, TOL_LEGACY, NEVER = range(6)


def cfg(bf, thr, F, crit=DIAMETER, tol=0.05, table=()):
    return dict(bf=bf, thr=thr, crit=crit, tol=tol, table=np.asarray(table, dtype=np.float64), F=F)


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------


def _prototypes(rng, F, k):
    return rng.random((k, F)) < 0.3


def rows_near(seed, n, F, k=4, flip=0.08):
    r"""n packed fingerprints, each one of k prototypes with `flip` of its bits inverted: they merge, append and split."""
    rng = np.random.default_rng(seed)
    proto = _prototypes(rng, F, k)
    bits = proto[rng.integers(0, k, n)] ^ (rng.random((n, F)) < flip)
    return np.packbits(bits, axis=1)


def bitfeatures(seed, ns, F, k=3, flip=0.1):
    r"""One BitFeature per entry of ns: ls[j] ~ Binomial(n, p_j) around one of k prototypes (p_j = 1 - flip on its bits,
    flip elsewhere), so ls[j] <= n always and a row of n == 1 is a 0/1 fingerprint.  -> (ls, n) as uint64."""
    rng = np.random.default_rng(seed)
    ns = np.asarray(ns, dtype=np.uint64)
    proto = _prototypes(rng, F, k)
    p = np.where(proto[rng.integers(0, k, ns.size)], 1.0 - flip, flip)
    ls = rng.binomial(ns[:, None].astype(np.int64), p).astype(np.uint64)
    return ls, ns


def table(ls, ns, width):
    t = np.concatenate([ls, ns[:, None]], axis=1)
    assert int(t.max()) <= np.iinfo(W[width]).max
    return np.ascontiguousarray(t.astype(W[width]))


def singleton_runs(n_col) -> list[int]:
    r"""Lengths of the maximal runs of n_samples == 1, in order."""
    runs, cur = [], 0
    for v in np.asarray(n_col).tolist():
        if v == 1:
            cur += 1
        elif cur:
            runs.append(cur)
            cur = 0
    if cur:
        runs.append(cur)
    return runs


# ---------------------------------------------------------------------------------------------------------------------
# 1. bbh_tree_fit_buffers: singleton runs around kMinRun = 1024 (width 1, F = 64)
# ---------------------------------------------------------------------------------------------------------------------

RUN_F = 64
RUN_CFG = cfg(6, 0.6, RUN_F)
# ("s", length): singletons; ("m", length): BitFeatures of 2..255 members.  RUN_LONG: the runs of >= 1024 the splitter packs.
RUN_TABLES = {
    "mixed": [("m", 3), ("s", 1023), ("m", 2), ("s", 1024), ("m", 4), ("s", 1025), ("m", 1), ("s", 2100), ("m", 2)],
    "starts_long": [("s", 1500), ("m", 5), ("s", 10), ("m", 3)],
    "ends_long": [("m", 4), ("s", 7), ("m", 2), ("s", 1300)],
    "one_run": [("s", 1100)],
    "no_singleton": [("m", 300)],
    # buffers, 1023 singletons that stay with them, one buffer, then a run the scan has to step back from (hi -= run1)
    "rewind": [("m", 6), ("s", 1023), ("m", 1), ("s", 1030), ("m", 2)],
}
RUN_LENGTHS = {name: [ln for kind, ln in spec if kind == "s"] for name, spec in RUN_TABLES.items()}


def run_ns(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    parts = [np.ones(ln, np.uint64) if kind == "s" else rng.integers(2, 256, ln).astype(np.uint64) for kind, ln in RUN_TABLES[name]]
    return np.concatenate(parts)


def run_table(name):
    ls, ns = bitfeatures(100 + sum(map(ord, name)), run_ns(name), RUN_F)
    return table(ls, ns, 1)


# ---------------------------------------------------------------------------------------------------------------------
# 1b. the other widths: the same BitFeatures as uint8 / 16 / 32 / 64 tables, the tier boundaries, pairs that merge across them
# ---------------------------------------------------------------------------------------------------------------------

TIER_F = 64
TIER_CFG = cfg(5, 0.3, TIER_F)
TIER_PAIRS = (200, 40000)  # 200 + 200 crosses 255 (uint8 -> uint16 tier), 40000 + 40000 crosses 65535 (uint16 -> uint32)
TIER_MAX_N = {1: 255, 2: 65535, 4: 65536, 8: 65536}


def tier_table(width):
    r"""-> (table, pairs): rows whose n_samples fits `width`; pairs = [(row a, row b, n)] of identical BitFeatures of n
    identical members each (ls = n * bits, a pattern of their own), adjacent, so that b merges into a."""
    rng = np.random.default_rng(77)
    ns = np.concatenate([np.ones(150, np.uint64), rng.integers(2, 256, 150).astype(np.uint64)])
    ns = ns[rng.permutation(ns.size)]
    ls, ns = bitfeatures(78, ns, TIER_F)
    special_ls, special_ns = bitfeatures(79, [255, 256, 65535, 65536], TIER_F)
    rows_ls, rows_ns, pairs = [ls[:200]], [ns[:200]], []
    at = 200
    for n in TIER_PAIRS + (255, 256, 65535, 65536):
        if n > TIER_MAX_N[width]:
            continue
        if n in TIER_PAIRS:
            bits = (rng.random(TIER_F) < 0.5).astype(np.uint64)
            rows_ls.append(np.stack([bits * n, bits * n]))
            rows_ns.append(np.array([n, n], np.uint64))
            pairs.append((at, at + 1, n))
            at += 2
        else:
            i = [255, 256, 65535, 65536].index(n)
            rows_ls.append(special_ls[i:i + 1])
            rows_ns.append(special_ns[i:i + 1])
            at += 1
    rows_ls.append(ls[200:])
    rows_ns.append(ns[200:])
    return table(np.concatenate(rows_ls), np.concatenate(rows_ns), width), pairs


# pool growth: a first call of width 8 whose buffers (2..255 members, hardly any merges) each take a uint8 slot
POOL_CFG = cfg(8, 0.95, 64)


def pool_table():
    rng = np.random.default_rng(5)
    return table(*bitfeatures(6, rng.integers(2, 256, 3000), 64, k=6, flip=0.2), 8)


RANGE_CFG = cfg(5, 0.5, 64)


def range_tables():
    r"""-> (ten valid rows and one of n_samples = 2^32, a small valid table for after the reset), width 8."""
    ls, ns = bitfeatures(8, [1, 2, 3, 1, 9, 200, 1, 1, 70, 4], 64)
    bad = np.concatenate([ls, np.full((1, 64), 1 << 31, np.uint64)]), np.concatenate([ns, np.array([1 << 32], np.uint64)])
    t = np.ascontiguousarray(np.concatenate([bad[0], bad[1][:, None]], axis=1))
    return t, table(*bitfeatures(9, [1, 5, 1, 1, 30, 2, 1, 300, 1, 1, 1, 7] * 5, 64), 8)


# every insertion kernel that takes buffers: F = 2048, bf 50 and 254, a width-1 table (with singleton runs the splitter packs)
# and the same BitFeatures at width 4
SWITCH_F = 2048
SWITCHES = ("", "BBHIP_NO_FAST", "BBHIP_NO_PIPE", "BBHIP_NO_SINGLETON_PATH")
SWITCH_SPEC = [("m", 500), ("s", 1500), ("m", 500), ("s", 500)]


def switch_cfg(bf):
    return cfg(bf, 0.5, SWITCH_F)


def switch_table(width):
    rng = np.random.default_rng(11)
    ns = np.concatenate([np.ones(ln, np.uint64) if kind == "s" else rng.integers(2, 256, ln).astype(np.uint64) for kind, ln in SWITCH_SPEC])
    return table(*bitfeatures(12, ns, SWITCH_F, k=400, flip=0.03), width)


# ---------------------------------------------------------------------------------------------------------------------
# 2. bbh_tree_fit_packed
# ---------------------------------------------------------------------------------------------------------------------

STRIDE_CFG = cfg(4, 0.5, 64)
STRIDE_EXTRA = (1, 4, 8)  # row_stride = nbytes + 1, nbytes + 4, 2 * nbytes
STRIDE_SLAB_KB = 1        # rows per slab = 1024 // row_stride


def stride_rows(extra, slabs):
    r"""Rows for a view of `slabs` slabs whose last slab (beyond the first) holds one row."""
    per = (STRIDE_SLAB_KB * 1024) // (8 + extra)
    n = per if slabs == 1 else (slabs - 1) * per + 1
    return rows_near(300 + extra, n, 64, k=30)


def strided_view(rows, stride, fill=0xA5):
    r"""A view of row stride `stride` whose last row ends exactly where the allocation ends; the gaps hold `fill`."""
    n, nb = rows.shape
    base = np.full((n - 1) * stride + nb, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(base, (n, nb), (stride, 1))
    view[:] = rows
    assert view.ctypes.data + (n - 1) * stride + nb == base.ctypes.data + base.nbytes
    return base, view


MISALIGNED_CFG = cfg(50, 0.5, 2048)
MISALIGNED = [(1, 260), (4, 264), (16, 272), (16, 264), (1, 272)]  # (base offset, row stride): only (16, 272) is 16-aligned


def misaligned_rows():
    return rows_near(41, 500, 2048, k=200, flip=0.03)


CHAIN_CFG = cfg(4, 0.5, 64)

# (bf, F) corners; bf 2 with a low threshold: most rows merge and the tree stays shallow
CORNERS = [(2, 8), (2, 8192), (1023, 8), (1023, 8192)]


def corner_case(bf, F):
    return cfg(bf, 0.3 if bf == 2 else 0.5, F), rows_near(500 + bf + F, 300, F, k=20 if bf == 2 else 40, flip=0.05)


THRESHOLD_CASES = {0.0: cfg(4, 0.0, 64), 1.0: cfg(4, 1.0, 64)}


def threshold_rows():
    r = rows_near(61, 200, 64, k=5, flip=0.02)
    return np.concatenate([r, r[:50]])  # exact repeats: the only merges at threshold 1.0


TOL_TABLE = [0.3, 0.2, 0.1, 0.05, 0.02]  # tol_len = 5: a cluster of five and more members reads 0


def tol_cases():
    return {
        "tol_diameter": cfg(5, 0.4, 64, TOL_DIAMETER, 0.05, TOL_TABLE),
        "tol_radius": cfg(5, 0.4, 64, TOL_RADIUS, 0.05, TOL_TABLE),
        "tol_diameter_null": cfg(5, 0.4, 64, TOL_DIAMETER, 0.05, ()),
        "tol_radius_null": cfg(5, 0.4, 64, TOL_RADIUS, 0.05, ()),
    }


def tol_rows():
    return rows_near(71, 400, 64, k=20, flip=0.05)


# ---------------------------------------------------------------------------------------------------------------------
# 3. mixed launches: per tree (cfg, history before the call, this call's input); the GPU file decides residency
# ---------------------------------------------------------------------------------------------------------------------


def mixed_packed():
    r"""Trees of one bbh_trees_fit_packed call: name -> (cfg, ops before the call, rows of the call or None for n = 0)."""
    big = lambda seed, n, k=150: rows_near(seed, n, 2048, k=k, flip=0.03)
    return {
        "bf50_fitted": (cfg(50, 0.5, 2048), [("packed", big(1, 600))], big(2, 700)),
        "bf254_fresh": (cfg(254, 0.5, 2048, TOL_DIAMETER, 0.05, TOL_TABLE), [], big(3, 900, 600)),
        "bf5_reset": (cfg(5, 0.5, 64, RADIUS), [("packed", rows_near(4, 300, 64, k=40)), ("reset",)], rows_near(5, 400, 64, k=40)),
        "bf17_strided": (cfg(17, 0.55, 800, TOL_RADIUS, 0.05, TOL_TABLE), [], rows_near(6, 500, 800, k=80, flip=0.05)),
        "empty": (cfg(50, 0.5, 2048), [("packed", big(7, 300))], None),
    }


def mixed_buffers():
    r"""Trees of one bbh_trees_fit_buffers call: name -> (cfg, ops before, table), widths 1, 2, 4 and 8 in one call."""
    def tab(seed, n, F, width, k=6):
        rng = np.random.default_rng(seed)
        ns = np.where(rng.random(n) < 0.5, 1, rng.integers(2, 256, n)).astype(np.uint64)
        return table(*bitfeatures(seed + 1, ns, F, k=k, flip=0.04 if F > 64 else 0.1), width)
    return {
        "bf50_w1_fitted": (cfg(50, 0.5, 2048), [("buffers", tab(21, 300, 2048, 1, 150))], tab(23, 500, 2048, 1, 150)),
        "bf254_w4_fresh": (cfg(254, 0.5, 2048), [], tab(25, 900, 2048, 4, 700)),
        "bf5_w2_reset": (cfg(5, 0.5, 64, RADIUS), [("buffers", tab(27, 200, 64, 2, 40)), ("reset",)], tab(29, 400, 64, 2, 40)),
        "bf17_w8": (cfg(17, 0.55, 800, TOL_RADIUS, 0.05, TOL_TABLE), [], tab(31, 400, 800, 8, 80)),
        "empty": (cfg(5, 0.5, 64), [("buffers", tab(33, 100, 64, 1))], None),
    }


# ---------------------------------------------------------------------------------------------------------------------
# 4. export / gather: singletons, the three tiers, several leaf nodes under an internal root
# ---------------------------------------------------------------------------------------------------------------------

GATHER_CFG = cfg(4, 0.6, 64)


def gather_ops():
    ls, ns = bitfeatures(91, [1, 1, 7, 1, 300, 1, 70000, 2, 1, 1, 40, 1, 500, 1, 1, 90000, 3, 1, 1, 1, 260, 1, 9, 1], 64, k=12, flip=0.08)
    return [("packed", rows_near(90, 12, 64, k=6)), ("buffers", table(ls, ns, 8))]


def position_sets(k):
    rng = np.random.default_rng(3)
    return {
        "reversed": np.arange(k - 1, -1, -1, dtype=np.int64),
        "shuffled": rng.permutation(k).astype(np.int64),
        "repeats": rng.integers(0, k, 3 * k).astype(np.int64),
        "first_last": np.array([0, k - 1], np.int64),
        "one": np.array([k // 2], np.int64),
    }


CHUNK_CFG = cfg(3, 0.9, 8)
CHUNK_M = (1 << 22) + 5  # gather() launches 2^22 rows at a time


def chunk_ops():
    # (the repeats come first: they merge while the root is still a leaf)
    rows = np.array([[0x01], [0x01], [0x02], [0x02], [0x04], [0x08], [0x10], [0x20], [0x40], [0x80], [0x03], [0x0C]], np.uint8)
    return [("packed", rows)]


# ---------------------------------------------------------------------------------------------------------------------
# 5. set_merge / reset
# ---------------------------------------------------------------------------------------------------------------------

MERGE_CFG = cfg(4, 0.35, 64, TOL_DIAMETER, 0.05, TOL_TABLE)
MERGE_NEW = (RADIUS, 0.0, (), 0.75)  # criterion, tolerance, table, threshold of the second fit


def merge_rows(i):
    return rows_near(800 + i, 300, 64, k=40, flip=0.08)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle driver
# ---------------------------------------------------------------------------------------------------------------------


def snapshot(eng, positions=None, width=8) -> dict:
    ids, ns, cents, ls = eng.export_leaves(ls_width=8)
    snap = dict(leaf_count=eng.leaf_count(), ids=ids, ns=ns, cents=cents, ls=ls.astype(np.uint64),
                stats=np.asarray(eng.stats()[:7], dtype=np.uint64))
    if positions is not None:
        snap["gathered"] = eng.gather_buffers(positions, width)
    return snap


def make_oracle(c) -> OracleEngine:
    return OracleEngine(c["bf"], c["thr"], c["crit"], c["tol"], c["table"], c["F"])


def apply_op(eng, op):
    r"""One operation on an engine with OracleEngine's methods -> out_leaf of a fit, else None."""
    if op[0] == "packed":
        return eng.fit_packed(op[1])
    if op[0] == "buffers":
        return eng.fit_buffers(op[1])
    if op[0] == "set_merge":
        return eng.set_merge(op[1], op[2], np.asarray(op[3], dtype=np.float64), op[4], op[5])
    if op[0] == "reset":
        return eng.reset()
    if op[0] == "compact":
        return eng.compact(op[1])
    if op[0] == "reload":
        return eng.reload()
    raise ValueError(op[0])


def run(eng, ops, positions=None, width=8) -> dict:
    r"""The operations on any engine with OracleEngine's methods -> its snapshot and the out_leaf of every fit."""
    out = [apply_op(eng, op) for op in ops]
    snap = snapshot(eng, positions, width)
    snap["out_leaf"] = [o for o in out if isinstance(o, np.ndarray)]
    return snap


def replay(c, ops, positions=None, width=8) -> dict:
    eng = make_oracle(c)
    snap = run(eng, ops, positions, width)
    eng.close()
    return snap


def same(got: dict, want: dict) -> None:
    r"""Everything observable is equal, exactly."""
    assert got["leaf_count"] == want["leaf_count"]
    for key in ("ids", "ns", "cents", "ls", "stats", "gathered"):
        if key in want:
            assert got[key].shape == want[key].shape and (got[key] == want[key]).all(), key
    assert len(got["out_leaf"]) == len(want["out_leaf"])
    for i, (a, b) in enumerate(zip(got["out_leaf"], want["out_leaf"])):
        assert a.shape == b.shape and (a == b).all(), f"out_leaf of fit {i}: first difference at {int(np.argmax(a != b))}"


def snapshot_rows(snap) -> np.ndarray:
    r"""The leaves of a snapshot as width-8 buffer rows [linear_sum | n_samples]."""
    return np.concatenate([snap["ls"], snap["ns"][:, None]], axis=1)
