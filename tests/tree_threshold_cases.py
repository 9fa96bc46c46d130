r"""Cases that put the tree engine's merge decisions and row choices ON their edges: pure data and builders, no GPU and no
library but the oracle.  test_tree_threshold_cases.py holds every case against the condition that makes it worth running, on
the C oracle alone (its bbo_tree_edge_counts says how many decisions compared two equal float64 values, how many best-row
searches ended in a tie); test_hip_tree_thresholds.py replays the same cases on libbbhip.so and compares with ==.

Isomorphic families.  A family has a core of c bits; each member adds p private bits; all of them disjoint inside the family,
at positions drawn per family.  For ANY n >= 2 members of one family the exact moments give
    a = n (n - 1) c / 2,   d = a + n (n - 1) p,   iSIM = a / d = c / (c + 2 p)
so every merge inside a family is decided at fl(c / (c + 2 p)) exactly, with other operands for threshold * d every time.  With
the threshold at q = fl(c / (c + 2 p)) every such decision is a comparison of two equal values; one ulp above it none merges.

Block rows.  The 2048 features are 32 blocks of 64 bits and a row is a union of whole blocks, so every popcount, intersection
and union is 64 times a small integer and Tanimoto ties between different (inter, union) pairs (1/6 = 2/12) are plentiful at
the widths the steady-state and pipelined kernels take."""
from __future__ import annotations

import functools

import numpy as np

import tree_abi_cases as T
from oracle_engine import oracle_lib
from tree_abi_cases import DIAMETER, RADIUS, TOL_DIAMETER, TOL_LEGACY, TOL_RADIUS  # noqa: F401

F = 2048
ORDERS = ("grouped", "shuffled", "interleaved")


def ulps(x: float, k: int) -> float:
    r"""The float64 k ulps above (k < 0: below) a positive x."""
    bits = np.array([x], np.float64).view(np.int64)
    assert bits[0] > 0 and bits[0] + k > 0
    return float((bits + k).view(np.float64)[0])


def q_of(c: int, p: int) -> float:
    return c / (c + 2 * p)  # one correctly rounded division: fl(c / (c + 2 p))


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------


def _family_bits(rng, m, c, p, n_features):
    r"""(m, n_features) bool: m members of one family."""
    assert c + m * p <= n_features
    pos = rng.permutation(n_features)[:c + m * p]
    bits = np.zeros((m, n_features), bool)
    bits[:, pos[:c]] = True
    bits[np.repeat(np.arange(m), p), pos[c:]] = True
    return bits


def _ordered(rng, blocks, order):
    r"""blocks: list of (m_i, F) arrays.  grouped: block after block; interleaved: member 0 of every block, member 1, ...;
    shuffled: a random permutation of all rows."""
    assert order in ORDERS
    if order == "interleaved":
        longest = max(b.shape[0] for b in blocks)
        return np.concatenate([b[i:i + 1] for i in range(longest) for b in blocks if i < b.shape[0]])
    rows = np.concatenate(blocks)
    return rows[rng.permutation(rows.shape[0])] if order == "shuffled" else rows


def families(seed, k, m, c, p, order="grouped", n_features=F):
    r"""k families of m members, packed: (k * m, n_features / 8) uint8."""
    rng = np.random.default_rng(seed)
    return np.packbits(_ordered(rng, [_family_bits(rng, m, c, p, n_features) for _ in range(k)], order), axis=1)


def mixed(seed, k, m, c, p, dup_runs=(300, 40, 40, 7, 300, 40), n_features=F):
    r"""On-edge families (c, p) between tight ones (p = 1: c / (c + 2), above the threshold), loose ones (p = 2 c: 1 / 5, below
    it) and runs of exact duplicates (iSIM 1; the runs of 300 cross the 255 -> 256 member tier promotion).  2 k families in
    all, half of them on the edge, the blocks grouped and in random order: at q + ulps the tree still merges (tight families,
    duplicates), appends, splits and promotes tiers."""
    rng = np.random.default_rng(seed)
    blocks = []
    for i in range(k):
        blocks.append(_family_bits(rng, m, c, p, n_features))
        blocks.append(_family_bits(rng, m, c, 1 if i % 2 == 0 else 2 * c, n_features))
    for run in dup_runs:
        blocks.append(np.repeat(_family_bits(rng, 1, c, p, n_features), run, axis=0))
    blocks = [blocks[i] for i in rng.permutation(len(blocks))]
    return np.packbits(np.concatenate(blocks), axis=1)


def with_tier_block(seed, k, m, c, p, big, at, n_features=F):
    r"""Grouped families with one family of `big` members as block number `at`: its on-edge merges cross 255 -> 256 members."""
    rng = np.random.default_rng(seed)
    blocks = [_family_bits(rng, big if i == at else m, c, p, n_features) for i in range(k)]
    return np.packbits(np.concatenate(blocks), axis=1), sum(b.shape[0] for b in blocks[:at])


def block_rows(seed, n, protos=200, lo=2, hi=6, swap=(1, 2), n_features=F, block=64):
    r"""n rows that are unions of whole `block`-bit blocks: one of `protos` planted prototypes (lo..hi blocks) with one or two
    of its blocks swapped for others."""
    rng = np.random.default_rng(seed)
    nblk = n_features // block
    sets = [rng.permutation(nblk)[:rng.integers(lo, hi + 1)] for _ in range(protos)]
    on = np.zeros((n, nblk), bool)
    for i in range(n):
        s = sets[rng.integers(0, protos)]
        row = np.zeros(nblk, bool)
        row[s] = True
        for _ in range(rng.integers(swap[0], swap[1] + 1)):
            row[rng.choice(np.flatnonzero(row))] = False
            row[rng.choice(np.flatnonzero(~row))] = True
        on[i] = row
    return np.packbits(np.repeat(on, block, axis=1), axis=1)


@functools.lru_cache(maxsize=None)
def criterion_value(crit, step, c=12, p=4):
    r"""The recurring value of a criterion at the step to new_n = `step` inside a family (the same in every family: they are
    isomorphic), from the oracle's functions on the column sums of the first `step` members of one family."""
    lib = oracle_lib()
    bits = _family_bits(np.random.default_rng(1), step, c, p, 256)
    ls = np.ascontiguousarray(bits.sum(axis=0), dtype=np.uint64)
    fn = lib.bbo_isim_from_sum if crit in (DIAMETER, TOL_DIAMETER, TOL_LEGACY) else lib.bbo_isim_radius_compl_from_sum
    return float(fn(ls.ctypes.data, ls.size, step))


def cut(rows, parts):
    r"""-> the operations that insert `rows` in `parts` fit_packed calls of unequal, odd lengths."""
    n = rows.shape[0]
    at = [0] + [(n * (2 * i + 1)) // (2 * parts) | 1 for i in range(1, parts)] + [n]
    return [("packed", np.ascontiguousarray(rows[a:b])) for a, b in zip(at[:-1], at[1:])]


# ---------------------------------------------------------------------------------------------------------------------
# the cases.  A case: name -> (cfg, ops).  Every builder is cached; nothing mutates what it returns.
# ---------------------------------------------------------------------------------------------------------------------

LADDER = (0, 1, -1, 8, -8, 24, -24, 40, -40, 1000, -1000)  # ulps around q: the 2^-48 band of bb_tree_pipe.inc is 16 - 32 wide
SHORT_LADDER = (0, 1, -1, 24, -40)
# (c, p): 1/3, 3/7, 5/9, 7/11 have inexact quotients, 1/2 an exact one
FRACTIONS = {"1/3": (12, 12), "3/7": (12, 8), "5/9": (10, 4), "7/11": (14, 4), "1/2": (8, 4)}

# Rows of the cases that must reach the pipelined kernel.  A fresh tree's first 8 192 elements belong to the steady-state
# kernel and the pipelined one takes all the rest (measured: kernel counts [n - 8 192, 8 192, 0] in every case), so condition
# (c), kc[0] > kc[1] + kc[2], holds from n = 16 385 on.  The cases take PIPE_K * PIPE_M = 24 000 rows: a round
# count at which the pipelined kernel's own share, the rows after the first 8 192, holds 1 000 on-edge decisions in every order
# (measured: shuffled 1 007, interleaved 1 077, mixed 7 382, grouped 14 988; test_tree_threshold_cases.py asserts it).
PIPE_K, PIPE_M = 1200, 20


@functools.lru_cache(maxsize=None)
def pipe_rows(frac, order="grouped"):
    c, p = FRACTIONS[frac]
    return families(1000 + sum(map(ord, frac)), PIPE_K, PIPE_M, c, p, order)


@functools.lru_cache(maxsize=None)
def mixed_rows(frac):
    c, p = FRACTIONS[frac]
    return mixed(2000 + sum(map(ord, frac)), PIPE_K // 2, PIPE_M, c, p)


def ladder_case(frac, bf, crit, off, kind="pure", order="grouped", table=()):
    r"""-> (cfg, ops): threshold q + off ulps, tolerance 0, three fit_packed calls."""
    rows = pipe_rows(frac, order) if kind == "pure" else mixed_rows(frac)
    return T.cfg(bf, ulps(q_of(*FRACTIONS[frac]), off), F, crit, 0.0, table), cut(rows, 3)


# which fraction climbs the whole ladder at which branching factor (diameter), and the shorter ladders
LADDER_PLAN = [("1/3", 50), ("3/7", 254), ("5/9", 50), ("1/2", 254)]
LADDER_CASES = (
    [(fr, bf, DIAMETER, off, "pure", "grouped") for fr, bf in LADDER_PLAN for off in LADDER]
    + [(fr, bf, TOL_DIAMETER, off, "pure", "grouped") for fr, bf in [("3/7", 50), ("5/9", 254)] for off in SHORT_LADDER]
    + [("7/11", 50, crit, off, "pure", "shuffled") for crit in (DIAMETER, TOL_DIAMETER) for off in (0, 1, -1)]
    + [("1/3", 254, DIAMETER, off, "pure", "interleaved") for off in (0, 24)]
    + [(fr, bf, crit, off, "mixed", "grouped") for fr, bf, crit in [("5/9", 50, DIAMETER), ("3/7", 254, TOL_DIAMETER), ("1/2", 50, TOL_DIAMETER)]
       for off in (0, 1, -24)]
)


def ladder_id(case):
    fr, bf, crit, off, kind, order = case
    return f"{fr}-bf{bf}-crit{crit}-{off:+d}ulp-{kind}-{order}"


# tolerance tables around q (tolerance-diameter: old_dc == new_dc == q inside a family, so old_dc - table[nT] lands on new_dc,
# one ulp under it, one ulp over it).  u = the ulp of q.
def tol_tables(q):
    u = ulps(q, 1) - q
    return {
        "empty": (),
        # nT = 2 reads 0.0 (on the edge, merges), nT = 3 reads +u (just under, merges), nT = 4 = tol_len - 1 reads -u (just
        # over: refused; a read of 0.0 or of a neighbour would merge).  A read one entry to either side refuses at 2 or at 3.
        "five": (-u, -u, 0.0, u, -u),
        # tol_len = 4: nT = 3 = tol_len - 1 reads +u, nT = 4 = tol_len and everything beyond reads 0.0: on the edge, merges
        "four": (-u, -u, 0.0, u),
        # (tolerance-radius: the criterion value falls with every member, and only a tolerance lets a cluster grow at all)
        "loose": (0.1,) * 16,
    }


TOL_DIAMETER_CASES = [(fr, bf, name) for fr, bf in [("5/9", 50), ("3/7", 254)] for name in ("five", "four")]


def tol_diameter_case(frac, bf, name):
    q = q_of(*FRACTIONS[frac])
    return T.cfg(bf, q, F, TOL_DIAMETER, 0.0, tol_tables(q)[name]), cut(pipe_rows(frac), 3)


# tier case: a family of 320 members (c, p = 10, 4: 1 290 bits) as block 700 of 1 200, after the steady-state kernel's first
# stretch: 65 on-edge merges with new_n > 255 (the `packed` branch of the pipelined kernel, `cold` in the steady-state one)
TIER_BIG = 320


@functools.lru_cache(maxsize=None)
def tier_rows():
    return with_tier_block(31, PIPE_K, PIPE_M, 10, 4, TIER_BIG, 700)


def tier_case(bf, crit, off=0):
    return T.cfg(bf, ulps(q_of(10, 4), off), F, crit, 0.0, ()), cut(tier_rows()[0], 2)


TIER_CASES = [(50, DIAMETER), (254, TOL_DIAMETER)]

# tolerance-legacy (steady-state kernel and complete engine): c, p = 12, 4, threshold q = fl(0.6); whether
# (q (n + 1) - q (n - 1)) / 2 < q - tolerance holds depends on n through rounding alone
LEGACY_K, LEGACY_M = 600, 20
LEGACY_TOLERANCES = (0.0, 1e-17, 1e-16, 1e-15)
LEGACY_CASES = [(bf, tol) for bf in (50, 254) for tol in LEGACY_TOLERANCES]


@functools.lru_cache(maxsize=None)
def legacy_rows():
    return families(41, LEGACY_K, LEGACY_M, 12, 4, "grouped")


def legacy_case(bf, tol):
    return T.cfg(bf, q_of(12, 4), F, TOL_LEGACY, tol, ()), cut(legacy_rows(), 2)


# radius criteria (complete engine only): 256 features, bf 5 and 17, 400 families of 20 members; threshold = the recurring
# criterion value of the step to new_n = 2, 3, 5, 9, at 0 and +-1 ulp
RADIUS_F, RADIUS_K, RADIUS_M = 256, 400, 20
RADIUS_STEPS = (2, 3, 5, 9)
# (tolerance-radius here with a table of 0.1 throughout, so that its first comparison decides as radius does; its second
# comparison and its table have cases of their own, TOLRAD_CASES)
RADIUS_CASES = [(bf, crit, step, off, tab) for bf in (5, 17) for crit, tab in [(RADIUS, "empty"), (TOL_RADIUS, "loose")]
                for step in RADIUS_STEPS for off in (0, 1, -1)]


@functools.lru_cache(maxsize=None)
def radius_rows(wide=False):
    return families(51, RADIUS_K, RADIUS_M, 12, 4, "grouped", F if wide else RADIUS_F)


def radius_case(bf, crit, step, off, tab="empty", wide=False):
    v = criterion_value(RADIUS, step)
    return T.cfg(bf, ulps(v, off), F if wide else RADIUS_F, crit, 0.0, tol_tables(v)[tab]), cut(radius_rows(wide), 2)


RADIUS_WIDE = [(50, RADIUS, 2, 0), (50, TOL_RADIUS, 3, 0)]  # radius_terms at 2048 bits

# tolerance-radius, the second comparison new_rc >= old_rc - table[nT].  Inside a family the criterion value of n members is
# v_n = criterion_value(RADIUS, n) and falls with n, so a singleton that joins nT members compares v_(nT + 1) with
# v_nT - table[nT]: the entry d_n = v_n - v_(n + 1) (exact: Sterbenz) lands old - tol ON new, d_n + u one ulp under it
# (merges), d_n - u one ulp over it (refused).  Entries 0 and 1 are never read (-1: a read one entry down refuses at nT = 2).
# The threshold is v_9, which no family cluster reaches: every comparison of equal values is the second one.  Runs of exact
# duplicates have the value 1 at every n: beyond tol_len they read 0.0 and merge on 1 >= 1 - 0.0, so clusters cross tol_len.
TOLRAD_DUP_RUN, TOLRAD_DUP_EVERY = 12, 10


def tolrad_tables(shift=0):
    v = lambda n: criterion_value(RADIUS, n)
    d = lambda n: v(n) - v(n + 1)
    u = ulps(v(3), 1) - v(3)
    tabs = {
        "none": (),
        # nT = 2 on, 3 under, 4 on, 5 = tol_len - 1 over: families stop at five members
        "six": (-1.0, -1.0, d(2), d(3) + u, d(4), d(5) - u),
        # nT = 2 on, 3 under, 4 = tol_len - 1 on; nT = 5 = tol_len reads 0.0: families stop at five, refused by the 0.0
        "five": (-1.0, -1.0, d(2), d(3) + u, d(4)),
        # bbh_tree_fit_buffers (chunks of 7, 1 and 5 members): nT = 7 on, nT = 8 = tol_len - 1 on for a buffer of five
        "chunks": (-1.0,) * 7 + (d(7), v(8) - v(13)),
    }
    # shift = +1 / -1: what a kernel that read table[nT + 1] / table[nT - 1] would see (test_tree_threshold_cases.py: it
    # changes the tree)
    return {k: (t[1:] if shift > 0 else (0.0,) + t if shift < 0 else t) for k, t in tabs.items()}


TOLRAD_CASES = [(bf, tab) for bf in (5, 17) for tab in ("six", "five")]
TOLRAD_WIDE = [(50, "six")]


@functools.lru_cache(maxsize=None)
def tolrad_rows(wide=False):
    n_features = F if wide else RADIUS_F
    rng = np.random.default_rng(53)
    blocks = []
    for i in range(RADIUS_K):
        blocks.append(_family_bits(rng, RADIUS_M, 12, 4, n_features))
        if i % TOLRAD_DUP_EVERY == 0:
            blocks.append(np.repeat(_family_bits(rng, 1, 12, 4, n_features), TOLRAD_DUP_RUN, axis=0))
    return np.packbits(np.concatenate(blocks), axis=1)


def tolrad_case(bf, tab, wide=False, shift=0):
    return (T.cfg(bf, criterion_value(RADIUS, 9), F if wide else RADIUS_F, TOL_RADIUS, 0.0, tolrad_tables(shift)[tab]),
            cut(tolrad_rows(wide), 2))

# ties: block rows, 24 000 of them (the pipelined kernel's majority, as above)
TIE_N = 24000
TIE_CASES = [(50, DIAMETER, 0.5), (254, TOL_DIAMETER, 0.5), (50, TOL_LEGACY, 0.5)]


@functools.lru_cache(maxsize=None)
def tie_rows():
    return block_rows(61, TIE_N)


def tie_case(bf, crit, thr):
    return T.cfg(bf, thr, F, crit, 0.0, ()), cut(tie_rows(), 3)


# bbh_tree_fit_buffers: every family is cut into chunks of 7, 1, 5, 4 and 3 members and each chunk is one BitFeature of the
# table, [column sums | members]: what the leaf of a tree fitted to that chunk at threshold q holds (test_tree_threshold_cases
# checks that against snapshot_rows of such a tree).  The chunks of a family follow one another (a family is found through
# its leaf node being the last one touched, as in the grouped row order: the tracking centroids above are all zero).  A chunk
# that meets its family's cluster gives the family's iSIM again: on-edge decisions with nS = 1, 5, 4, 3.  Width 4 adds families
# of 600 members cut 300 / 300: nS = 300 is wider than uint8 (tier_for(nS) != 0) and the merge crosses 255.  The radius
# criteria: threshold = the criterion value of the step to 7 + 1 + 5 = 13 members.
BUF_CHUNKS = (7, 1, 5, 4, 3)
BUF_C, BUF_P = 11, 3  # 11/17, inexact
BUF_BIG, BUF_BIG_EVERY = 600, 50
BUF_CASES = [(DIAMETER, 50), (TOL_DIAMETER, 254), (TOL_LEGACY, 50), (RADIUS, 5), (TOL_RADIUS, 17)]


def chunk_features(bits, sizes):
    r"""-> (len(sizes), F + 1) uint64: the BitFeature of every chunk of one family's members."""
    at = np.concatenate([[0], np.cumsum(sizes)])
    return np.stack([np.concatenate([bits[a:b].sum(axis=0), [b - a]]) for a, b in zip(at[:-1], at[1:])]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def buffer_table(radius, width):
    r"""-> the table, (k, F + 1) of `width` bytes."""
    n_features, k, c, p = (RADIUS_F, 400, 12, 4) if radius else (F, 400, BUF_C, BUF_P)
    rng = np.random.default_rng(71)
    parts = []
    for i in range(k):
        parts.append(chunk_features(_family_bits(rng, sum(BUF_CHUNKS), c, p, n_features), BUF_CHUNKS))
        if width > 1 and not radius and i % BUF_BIG_EVERY == BUF_BIG_EVERY // 2:
            parts.append(chunk_features(_family_bits(rng, BUF_BIG, c, p, n_features), (BUF_BIG // 2, BUF_BIG // 2)))
    tab = np.concatenate(parts)
    assert int(tab.max()) <= np.iinfo(T.W[width]).max
    return np.ascontiguousarray(tab.astype(T.W[width]))


def buffer_case(crit, bf, width):
    radius = crit in (RADIUS, TOL_RADIUS)
    tab = buffer_table(radius, width)
    if radius:
        v = criterion_value(RADIUS, sum(BUF_CHUNKS[:3]))
        c = T.cfg(bf, v, RADIUS_F, crit, 0.0, tolrad_tables()["chunks"] if crit == TOL_RADIUS else ())
    else:
        c = T.cfg(bf, q_of(BUF_C, BUF_P), F, crit, 0.0, ())
    at = (tab.shape[0] // 2) | 1
    return c, [("buffers", tab[:at]), ("buffers", tab[at:])]


# bbh_trees_fit_packed: three family trees at bf 254, another fraction each, one launch (each tree's rows in one piece)
MULTI_CASES = [("1/3", 254, DIAMETER, 0, "pure", "grouped"), ("3/7", 254, DIAMETER, 0, "pure", "grouped"), ("5/9", 254, TOL_DIAMETER, 0, "pure", "grouped")]

# BBHIP_TINY_POOLS: on-edge decisions replayed after a pool stop and relaunch
TINY_CASE = ("5/9", 50, DIAMETER, 0, "mixed", "grouped")


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's replay with its edge counters
# ---------------------------------------------------------------------------------------------------------------------


def compact(snap):
    r"""A snapshot whose linear sums (leaves x features uint64, nearly all zero: 390 MB for 24 000 leaves) are held as their
    non-zero entries; `expand` gives them back.  What is cached and what a child process writes is compact."""
    ls = snap["ls"]
    nz = np.flatnonzero(ls)
    val = ls.reshape(-1)[nz]
    assert ls.size < 2**32 and int(val.max(initial=0)) < 2**32
    rest = {k: v for k, v in snap.items() if k != "ls"}
    return dict(rest, ls_nz=nz.astype(np.uint32), ls_val=val.astype(np.uint32), ls_shape=np.array(ls.shape, np.int64))


def expand(snap):
    ls = np.zeros(int(np.prod(snap["ls_shape"])), np.uint64)
    ls[snap["ls_nz"]] = snap["ls_val"]
    rest = {k: v for k, v in snap.items() if not k.startswith("ls_")}
    return dict(rest, ls=ls.reshape(tuple(int(v) for v in snap["ls_shape"])))


def replay(c, ops):
    r"""tree_abi_cases.replay, compact, with snap["edge"] = OracleEngine.edge_counts() and snap["walk"] = the pre-order walk
    without its linear sums (test_edge_reference.py holds it against the reference's tree, internal nodes included)."""
    eng = T.make_oracle(c)
    snap = T.run(eng, ops)
    snap["edge"] = eng.edge_counts()
    snap["tie_depths"] = eng.tie_depths()
    snap["walk"] = eng.walk(ls=False)
    eng.close()
    return compact(snap)


BUILDERS = {"ladder": ladder_case, "tol": tol_diameter_case, "tier": tier_case, "legacy": legacy_case, "radius": radius_case,
            "tie": tie_case, "buffers": buffer_case, "tolrad": tolrad_case}


def build(kind, *args):
    r"""-> (cfg, ops) of a case."""
    return BUILDERS[kind](*args)


@functools.lru_cache(maxsize=None)
def replay_named(kind, *args):
    r"""The oracle's replay of a case, computed once per process."""
    return replay(*build(kind, *args))


# the cases that run under every kernel switch (2048 bits, bf 50 / 254), in one child process per switch
SWITCH_CASES = ([("ladder",) + c for c in LADDER_CASES] + [("tol",) + c for c in TOL_DIAMETER_CASES] + [("tier",) + c for c in TIER_CASES]
                + [("legacy",) + c for c in LEGACY_CASES] + [("tie",) + c for c in TIE_CASES])


def case_id(case):
    return (ladder_id(case[1:]) if case[0] == "ladder" else "-".join(str(v) for v in case)).replace("/", "_")


def case_criterion(case):
    return {"ladder": lambda a: a[2], "tol": lambda a: TOL_DIAMETER, "tier": lambda a: a[1], "legacy": lambda a: TOL_LEGACY,
            "tie": lambda a: a[1]}[case[0]](case[1:])
