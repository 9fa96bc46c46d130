r"""Routing a fingerprint through a fitted tree without inserting it (bbh_tree_route_packed, BitBirch.route): the NumPy reference
and the cases, pure data and builders, no GPU and no library but the oracle.  TEST INFRASTRUCTURE - never imported by the product.

The reference walks OracleEngine.walk() (the whole tree in pre-order) with tree_image_format.walk_children: from the root, the
first argmax of i / max(u, 1) over the node's rows, decided on exact integers, down to a leaf row; there bbo_merge_accept on
the row's linear sum and the query as a nominee of one fingerprint.  test_route_refs.py holds it against the oracle itself
(rebuild the tree, insert the row alone) and every case against the condition it is named for; test_hip_route.py compares
libbbhip.so with it, ==.

A case: name -> (cfg, operations that build the tree (tree_abi_cases.apply_op), queries (m, F / 8) uint8)."""
from __future__ import annotations

import functools

import numpy as np

import tree_abi_cases as T
import tree_image_format as IMG
import tree_threshold_cases as TH
from oracle_engine import oracle_lib
from tree_abi_cases import DIAMETER, NEVER, RADIUS, TOL_DIAMETER, TOL_LEGACY, TOL_RADIUS

CRITERIA = {"diameter": DIAMETER, "radius": RADIUS, "tol_diameter": TOL_DIAMETER, "tol_radius": TOL_RADIUS, "tol_legacy": TOL_LEGACY, "never": NEVER}
TIERS = ("lazy", "uint8", "uint16", "uint32")  # the cluster features of a leaf row of n_samples 1, 2..255, 256..65535, above


def tier_of(n: int) -> int:
    return 0 if n == 1 else (1 if n <= 255 else (2 if n <= 65535 else 3))


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------


def first_argmax(i: np.ndarray, u: np.ndarray) -> tuple[int, bool, bool]:
    r"""-> (the first row whose i / max(u, 1) is the largest, by cross-multiplication of integers; whether that maximum is
    above 0 and attained by more than one row; whether the tied rows have different (i, u) pairs)."""
    i = i.astype(np.int64)
    u = np.maximum(u.astype(np.int64), 1)
    best = int(np.argmax(i / u))
    while True:  # (the float quotient is only a first guess: the decision is the integers')
        above = i * u[best] > i[best] * u
        if not above.any():
            break
        best = int(np.argmax(above))
    tied = np.flatnonzero(i * u[best] == i[best] * u)
    first = int(tied[0])
    many = i[first] > 0 and tied.size > 1
    return first, bool(many), bool(many and (len({(int(i[r]), int(u[r])) for r in tied}) > 1))


def route(walk: dict, c: dict, queries: np.ndarray) -> dict:
    r"""The reference: leaf (uint32 BitFeature id), accept (uint8), inter, union (uint32) per query, and what the walk met:
    depth (levels visited), ties / ties_differ (searches with a tied maximum / tied between different pairs), tier of the
    leaf row, lens (the lengths of the nodes visited)."""
    lib = oracle_lib()
    F = c["F"]
    nodes = walk["nodes"]
    assert len(nodes), "an empty tree routes nothing"
    row_start, children = IMG.walk_children(walk)
    pop, cent = walk["pop"].astype(np.int64), walk["cent"]
    tab = np.ascontiguousarray(c["table"], dtype=np.float64)
    m = queries.shape[0]
    out = dict(leaf=np.empty(m, np.uint32), accept=np.empty(m, np.uint8), inter=np.empty(m, np.uint32), union=np.empty(m, np.uint32),
               depth=np.empty(m, np.int64), ties=np.zeros(m, np.int64), ties_differ=np.zeros(m, np.int64), tier=np.empty(m, np.int64), lens=[])
    for e in range(m):
        q = queries[e]
        qbits = np.unpackbits(q)[:F].astype(np.uint64)
        pq = int(qbits.sum())
        k, depth = 0, 1
        while True:
            lo, hi = int(row_start[k]), int(row_start[k + 1])
            assert hi > lo, "a node without rows"
            inter = np.unpackbits(cent[lo:hi] & q, axis=1).sum(axis=1).astype(np.int64)
            union = pop[lo:hi] + pq - inter
            r, many, differ = first_argmax(inter, union)
            out["ties"][e] += many
            out["ties_differ"][e] += differ
            out["lens"].append(hi - lo)
            if nodes[k, 1]:
                break
            k = children[k][r]
            depth += 1
        row = lo + r
        old_n = int(walk["n"][row])
        old_ls = np.ascontiguousarray(walk["ls"][row], dtype=np.uint64)
        new_ls = np.ascontiguousarray(old_ls + qbits, dtype=np.uint64)
        if c["crit"] == NEVER or old_n + 1 > 0xFFFFFFFF:
            acc = 0
        else:
            acc = lib.bbo_merge_accept(c["crit"], c["thr"], c["tol"], tab.ctypes.data if tab.size else None, tab.size, new_ls.ctypes.data,
                                       old_n + 1, old_ls.ctypes.data, old_n, 1, F)
        out["leaf"][e], out["accept"][e], out["inter"][e], out["union"][e] = walk["id"][row], acc, inter[r], union[r]
        out["depth"][e], out["tier"][e] = depth, tier_of(old_n)
    return out


def build_oracle(c, ops):
    eng = T.make_oracle(c)
    for op in ops:
        T.apply_op(eng, op)
    return eng


def insert_alone(c, ops, row: np.ndarray) -> tuple[bool, int]:
    r"""The oracle itself: rebuild the tree, insert `row` alone -> (did it merge, its out_leaf)."""
    eng = build_oracle(c, ops)
    before = int(eng.stats()[2])
    leaf = eng.fit_packed(np.ascontiguousarray(row[None, :]))
    merged = int(eng.stats()[2]) - before
    eng.close()
    assert merged in (0, 1)
    return bool(merged), int(leaf[0])


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------


def _flip(rng, rows, bits, F):
    r"""Copies of packed rows with up to `bits` random bits inverted."""
    out = np.unpackbits(rows, axis=1)[:, :F].copy()
    for r in range(out.shape[0]):
        at = rng.integers(0, F, bits)
        out[r, at] ^= 1
    return np.packbits(out, axis=1)


@functools.lru_cache(maxsize=None)
def depth_case():
    r"""256-bit rows, bf 5, threshold 0.5, 600 rows in: four levels.  150 queries: 60 fresh rows around the tree's own
    prototypes, 60 around prototypes it never saw, 30 rows it holds."""
    c = T.cfg(5, 0.5, 256)
    rows = T.rows_near(11, 600, 256, k=40, flip=0.06)
    q = np.concatenate([T.rows_near(11, 700, 256, k=40, flip=0.06)[640:], T.rows_near(12, 60, 256, k=40, flip=0.06), rows[::20]])
    return c, (("packed", rows),), np.ascontiguousarray(q)


WIDTHS = (8, 104, 2048, 8192)
BFS = (2, 3, 50, 254, 1023)


@functools.lru_cache(maxsize=None)
def width_case(F, bf):
    r"""A few hundred rows at every (row width, branching factor) corner; bf 1023 with a never-merge tree of 600 rows: one leaf
    root of more than 512 rows (at 8 bits there are only 256 different rows: the trees of bf 50 and 254 stay one leaf).  40 queries: fresh rows of the same prototypes, rows of others, the all-zero and the all-one row."""
    never = bf == 1023
    c = T.cfg(bf, 0.3 if bf <= 3 else 0.5, F, NEVER if never else DIAMETER)
    n = 600 if never else (500 if bf == 254 else 300)
    k = {2: 20, 3: 20, 50: 400, 254: 600, 1023: 40}[bf]  # (bf 50 and 254: enough clusters for a root above the leaves)
    rows = T.rows_near(500 + bf + F, n, F, k=k, flip=0.05)
    q = np.concatenate([T.rows_near(500 + bf + F, n + 24, F, k=k, flip=0.05)[n:], T.rows_near(900 + bf + F, 14, F, k=k, flip=0.05),
                        np.zeros((1, F // 8), np.uint8), np.full((1, F // 8), 255, np.uint8)])
    return c, (("packed", rows),), np.ascontiguousarray(q)


LENGTHS = (1, 4, 5, 50)  # a leaf root of 1, 4, 5 and bf = bf + 1 - 1 rows


@functools.lru_cache(maxsize=None)
def length_case(n):
    c = T.cfg(50, 0.5, 104, NEVER)
    rows = T.rows_near(70 + n, n, 104, k=8, flip=0.1)
    return c, (("packed", rows),), np.ascontiguousarray(np.concatenate([T.rows_near(71 + n, 6, 104, k=8, flip=0.1), rows[:1]]))


@functools.lru_cache(maxsize=None)
def tie_case(name):
    r"""zero: the all-zero query (every similarity is 0: row 0 at every level) and an all-zero centroid row in the tree;
    dups: duplicated centroids (a never-merge tree of repeated rows) and queries equal to a centroid;
    halves: 1/2 against 2/4, either order; blocks: unions of 64-bit blocks at 2048 bits, ties between different pairs."""
    if name == "zero":
        c = T.cfg(4, 0.5, 64)
        rows = np.concatenate([np.zeros((1, 8), np.uint8), T.rows_near(31, 120, 64, k=12, flip=0.08)])
        q = np.concatenate([np.zeros((2, 8), np.uint8), T.rows_near(32, 10, 64, k=12, flip=0.08), np.eye(8, dtype=np.uint8)[:4]])
        return c, (("packed", rows),), np.ascontiguousarray(q)
    if name == "dups":
        c = T.cfg(4, 0.5, 64, NEVER)
        base = T.rows_near(33, 12, 64, k=12, flip=0.08)
        rows = np.repeat(base, 5, axis=0)[np.random.default_rng(34).permutation(60)]
        return c, (("packed", rows),), np.ascontiguousarray(np.concatenate([base, _flip(np.random.default_rng(35), base, 2, 64)]))
    if name == "halves":
        c = T.cfg(5, 0.5, 8, NEVER)
        a, b, q = 0b00000001, 0b00001111, 0b00000011  # a: 1 / 2, b: 2 / 4
        return c, (("packed", np.array([[a], [b], [0b11110000], [b], [a]], np.uint8)),), np.array([[q], [b], [a], [0b00000111]], np.uint8)
    assert name == "blocks"
    c = T.cfg(50, 0.5, 2048)
    rows = TH.block_rows(41, 900, protos=120)
    return c, (("packed", rows),), np.ascontiguousarray(TH.block_rows(42, 60, protos=120))


TIE_CASES = ("zero", "dups", "halves", "blocks")
CRIT_SHAPES = [(crit, 256, 5) for crit in CRITERIA] + [("diameter", 2048, 50), ("tol_radius", 2048, 50)]
CRIT_C, CRIT_P, CRIT_M = 12, 4, 5  # families of a 12-bit core and 4 private bits, 5 members in the tree: iSIM 12 / 20 inside
CRIT_TABLE = (0.3, 0.2, 0.1)       # shorter than old_n = 5: the tolerance of the edge decisions reads 0


@functools.lru_cache(maxsize=None)
def criterion_case(crit, F, bf):
    r"""Isomorphic families (tree_threshold_cases): 5 members of each are in the tree, a sixth and a seventh are queries, so
    that the decision is the family's recurring value against a threshold set to exactly that value (the criterion's value at
    the step to new_n = 6); families with 2 and 1 members in, whose decisions (new_n = 3, 2; old_n = 1: the early returns)
    are off it; and rows of no family.  The tolerance tables end at or before old_n = 5."""
    code = CRITERIA[crit]
    rng = np.random.default_rng(50 + code + F + bf)
    k = 24
    fams = [TH._family_bits(rng, CRIT_M + 2, CRIT_C, CRIT_P, F) for _ in range(k)]
    keep = [CRIT_M if f % 3 else 1 + (f // 3) % 2 for f in range(k)]  # (every third family: 1 or 2 members in)
    rows = np.packbits(np.concatenate([fam[:m] for fam, m in zip(fams, keep)]), axis=1)
    q = np.packbits(np.concatenate([fam[CRIT_M:] for fam in fams] + [rng.random((12, F)) < 0.05]), axis=1)
    if code == TOL_RADIUS:
        # (the value falls with every member: beyond the table - tolerance 0 - no family cluster grows, so the decisions on the
        # edge are the second comparison's, new_rc >= old_rc - table[2] with table[2] = v_2 - v_3 exactly, for the families
        # with two members in; the five-member clusters sit at old_n = tol_len and are refused by the 0.0 they read)
        c = T.cfg(bf, TH.criterion_value(RADIUS, 9, CRIT_C, CRIT_P), F, code, 0.0, TH.tolrad_tables()["five"])
    else:
        thr = TH.criterion_value(code if code != NEVER else DIAMETER, CRIT_M + 1, CRIT_C, CRIT_P)
        c = T.cfg(bf, thr, F, code, 0.05, CRIT_TABLE if code == TOL_DIAMETER else ())
    return c, (("packed", rows),), np.ascontiguousarray(q)


@functools.lru_cache(maxsize=None)
def tier_case(width=8):
    r"""Leaf rows of 1, 2..255, 256..65535 and more members, inserted as BitFeature buffers (tree_abi_cases.gather_ops);
    queries: every leaf's centroid with up to two bits inverted, and the centroid itself."""
    c = T.cfg(4, 0.6, 64)
    ops = tuple(T.gather_ops())
    eng = build_oracle(c, ops)
    cents = eng.export_leaves()[2]
    eng.close()
    return c, ops, np.ascontiguousarray(np.concatenate([_flip(np.random.default_rng(61), cents, 2, 64), cents]))


@functools.lru_cache(maxsize=None)
def storage_case(name):
    r"""Trees whose nodes get sealed: the depth case, and 2048-bit rows at bf 50 (a leaf-parent root over leaves)."""
    if name == "depth":
        return depth_case()
    c = T.cfg(50, 0.5, 2048)
    rows = T.rows_near(81, 1500, 2048, k=300, flip=0.03)
    return c, (("packed", rows),), np.ascontiguousarray(np.concatenate([T.rows_near(81, 1560, 2048, k=300, flip=0.03)[1500:], T.rows_near(82, 40, 2048, k=300, flip=0.03)]))


STORAGE_CASES = ("depth", "wide")
STORAGE_OPS = (("compact", 1), ("compact", 1), ("compact", 0), ("reload",))  # the queries run after the second, third and fourth

CASES = {"depth": depth_case}
CASES.update({f"width_{F}_bf{bf}": functools.partial(width_case, F, bf) for F in WIDTHS for bf in BFS})
CASES.update({f"length_{n}": functools.partial(length_case, n) for n in LENGTHS})
CASES.update({f"ties_{name}": functools.partial(tie_case, name) for name in TIE_CASES})
CASES.update({f"crit_{crit}_{F}_bf{bf}": functools.partial(criterion_case, crit, F, bf) for crit, F, bf in CRIT_SHAPES})
CASES.update({"tiers": tier_case, "storage_wide": functools.partial(storage_case, "wide")})


@functools.lru_cache(maxsize=None)
def expected(name) -> dict:
    r"""The reference's answer for a case (computed once, shared, never changed)."""
    c, ops, q = CASES[name]()
    eng = build_oracle(c, ops)
    walk = eng.walk()
    eng.close()
    res = route(walk, c, q)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    res["tree_depth"] = int(walk["nodes"][:, 0].max())
    res["node_lens"] = sorted(set(walk["nodes"][:, 2].tolist()))
    return res


class RefEngine:
    r"""An engine with HipEngine's face for the CPU tests of the Python surface: the oracle's tree, and `route_packed` by the
    reference above."""

    def __new__(cls, branching_factor, threshold, criterion, tolerance, tol_table, n_features, device=0):
        from oracle_engine import OracleEngine

        class _Ref(OracleEngine):
            def __init__(self, *a):
                super().__init__(*a)
                self._cfg = T.cfg(branching_factor, threshold, n_features, criterion, tolerance, tol_table)

            def set_merge(self, criterion, tolerance, tol_table, threshold, branching_factor):
                super().set_merge(criterion, tolerance, tol_table, threshold, branching_factor)
                self._cfg = T.cfg(branching_factor, threshold, self.n_features, criterion, tolerance, tol_table)

            def route_packed(self, rows, stream=None):
                rows = np.ascontiguousarray(rows, dtype=np.uint8)
                res = route(self.walk(), self._cfg, rows)
                return res["leaf"], res["accept"], res["inter"], res["union"]

        return _Ref(branching_factor, threshold, criterion, tolerance, tol_table, n_features, device)
