r"""Cases that put the tree engine's NODE SPLIT on its edges: pure data and builders, no GPU and no library but the oracle.
test_tree_split_cases.py holds every case against the conditions it names, on the C oracle alone (bbo_tree_split_counts says
what the splits of a replay met); test_hip_tree_splits.py replays the same cases on libbbhip.so and compares leaves, counters
and the whole tree image, internal nodes included, with ==.

Rows are unions of whole blocks of bits (32 blocks to a row at every width but 8192 bits, where there are more), so every
popcount, intersection and union is a small integer times the block size and a case can be worked out by hand.  A row is
written as the tuple of its block numbers.

Two camps.  Camp X: the core blocks 0, 1, 2 and `extra` of the blocks 3..8; camp Y: 12, 13, 14 and `extra` of 15..20; X and Y
alternate.  Under the never-merge criterion the first bf + 1 = m rows ARE the root when it splits.  With |X| = m / 2 every
core column is set in exactly half the rows: the majority vote (2 * count >= m) sets both cores, every row is equally far from
that centroid (the first argmin is row 0, an X row), fp2 is the first Y row and n1 == n2.  One row fewer in X and there is
neither a majority tie nor n1 == n2.

The second split.  After such a root split the X leaf (row 0 of the new root) holds m / 2 rows P = core + 2 extras.  More rows
for that leaf until it overflows: P rows, `s` rows Z = (2, 9) and - kind "gt" - one row Q = (0, 1, 21..26).  Similarities:
to the majority centroid (0, 1, 2): P 3/5, Z 1/4, Q 2/9.  Kind "le": fp1 is the first Z, P rows are 1/6 from it, fp2 is row 0,
the Z rows go to the new node: n1 = s <= n2 and the smaller half is the NEW node's.  Kind "gt": fp1 is Q, Z rows are 0 from it,
fp2 is the first Z, P rows are 2/11 from Q and 1/6 from Z and go with Q: n1 = m - s > n2 = s and the smaller half is the one
that STAYS.  Either way the smaller half is the s rows Z, the leaf is no root, and the engine computes the other tracking
BitFeature as old tracking sum + element - smaller half.  With n_samples on the rows (bbh_tree_fit_buffers: a BitFeature of n
identical members has ls = n * bits and the same centroid) the same rows carry every storage tier into the smaller half.
TEST INFRASTRUCTURE - never imported by the product."""
from __future__ import annotations

import functools

import numpy as np

import pipe_forward_cases as PF
import tree_abi_cases as T
import tree_threshold_cases as H
from tree_abi_cases import DIAMETER, NEVER

F = 2048
# bits per block at every width the cases use: 32 blocks to a row (2056 bits: 32 blocks of 64 and one byte that stays zero)
BLOCK = {64: 2, 256: 8, 512: 16, 1024: 32, 2048: 64, 2056: 64, 8192: 256}


def rows_of(sets, n_features=F) -> np.ndarray:
    r"""Packed rows, one per tuple of block numbers."""
    blk = BLOCK[n_features]
    bits = np.zeros((len(sets), n_features), bool)
    for i, s in enumerate(sets):
        for b in s:
            assert (b + 1) * blk <= n_features
            bits[i, b * blk:(b + 1) * blk] = True
    return np.ascontiguousarray(np.packbits(bits, axis=1))


def features_of(sets, ns, n_features=F, width=4) -> np.ndarray:
    r"""A buffer table [linear sum | n_samples]: row i is a BitFeature of ns[i] identical members."""
    bits = np.unpackbits(rows_of(sets, n_features), axis=1)[:, :n_features].astype(np.uint64)
    ns = np.asarray(ns, np.uint64)
    return T.table(bits * ns[:, None], ns, width)


X_CORE, Y_CORE = (0, 1, 2), (12, 13, 14)
Z, Q = (2, 9), (0, 1, 21, 22, 23, 24, 25, 26)


def camp_row(core, i, extra):
    r"""Member i of a camp: its core and `extra` of the six blocks behind it, in turn (every extra column is in at most a
    third of the camp)."""
    first = core[-1] + 1
    return core + tuple(sorted(first + (i + j) % 6 for j in range(extra)))


def two_camps(m, nx, extra=1, x_first=True):
    r"""m rows, nx of camp X and m - nx of camp Y, alternating from row 0 (the longer camp's rest at the end)."""
    sets, ix, iy = [], 0, 0
    for r in range(m):
        want_x = (r % 2 == 0) == x_first
        if (want_x and ix < nx) or iy >= m - nx:
            sets.append(camp_row(X_CORE, ix, extra))
            ix += 1
        else:
            sets.append(camp_row(Y_CORE, iy, extra))
            iy += 1
    assert ix == nx and iy == m - nx
    return sets


def never(bf, n_features=F):
    return T.cfg(bf, 0.5, n_features, NEVER, 0.0, ())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the crafted first split (the complete engine; never-merge)
# ---------------------------------------------------------------------------------------------------------------------

def camps_case(bf, nx, n_features=F):
    r"""The root's split over two camps, then eight more rows of both camps (they meet the two new tracking rows)."""
    m = bf + 1
    return never(bf, n_features), [("packed", rows_of(two_camps(m, nx), n_features)), ("packed", rows_of(two_camps(8, 4, 2), n_features))]


def three_camps(m, nx):
    r"""nx rows of camp X and m - nx of two other camps, Y1 = (12, 13, 14) and Y2 = (16, 17, 18) with one of four extra blocks
    each, in turn: X, Y1, X, Y2, ...  With nx = m / 2 the X core is the ONLY majority (by the tie), the first Y1 row is furthest
    from the centroid and becomes fp1; a vote that lost the tie would leave an empty centroid and row 0 as fp1.  (Two camps
    alone cannot tell: with both cores or neither in the centroid, row 0 is fp1 either way.)"""
    sets, ix, iy = [], 0, 0
    for r in range(m):
        if (r % 2 == 0 and ix < nx) or iy >= m - nx:
            sets.append(camp_row(X_CORE, ix, 1))
            ix += 1
        else:
            sets.append(((12, 13, 14, 24 + (iy // 2) % 4) if iy % 2 == 0 else (16, 17, 18, 28 + (iy // 2) % 4)))
            iy += 1
    assert ix == nx and iy == m - nx
    return sets


def camps3_case(bf, nx, n_features=F):
    m = bf + 1
    return never(bf, n_features), [("packed", rows_of(three_camps(m, nx), n_features)), ("packed", rows_of(three_camps(8, 4), n_features))]


TIE3 = dict(majority_tie=True, argmin1_tie=True, root=True, n1_eq_n2=False)
TIE = dict(majority_tie=True, n1_eq_n2=True, argmin1_tie=True, root=True)
NO_TIE = dict(majority_tie=False, n1_eq_n2=False, root=True)
CAMP_BF = (3, 63, 123, 125, 127, 255, 1023)  # m = 4, 64, 124, 126, 128, 256, 1024
ODD_BF = (64, 124, 128)                      # m = 65, 125, 129: no tie possible, floor(m / 2) and ceil(m / 2) on either side


def node_case(kind, bf=63, n_features=F):
    r"""Whole nodes of one kind, m = bf + 1 rows, then four more rows.
    duplicates: m equal rows - every similarity is 1, fp1 == fp2 == row 0, only fp1 leaves (n1 = 1: `|| r == fp1`)
    zeros: m all-zero rows - every union is 0 (max(union, 1)), every similarity 0, the same outcome
    one_zero: one all-zero row among X rows: it is fp1, all similarities to it are 0, fp2 is row 0
    fp1_last / fp1_first: X rows and one Y row as the last row / as row 0: the outlier is fp1"""
    m = bf + 1
    x = [camp_row(X_CORE, i, 1) for i in range(m)]
    sets = {"duplicates": [X_CORE + (5,)] * m, "zeros": [()] * m, "one_zero": x[:m // 3] + [()] + x[m // 3 + 1:],
            "fp1_last": x[:-1] + [Y_CORE + (15,)], "fp1_first": [Y_CORE + (15,)] + x[1:]}[kind]
    more = {"duplicates": [X_CORE + (5,)] * 4, "zeros": [()] * 4}.get(kind, x[:2] + [Y_CORE + (15,), ()])
    return never(bf, n_features), [("packed", rows_of(sets, n_features)), ("packed", rows_of(more, n_features))]


NODE_KINDS = {"duplicates": dict(fp1_is_fp2=True, argmin1_tie=True, argmin2_tie=True, equal_sims=True),
              "zeros": dict(fp1_is_fp2=True, zero_row=True, equal_sims=True),
              "one_zero": dict(zero_row=True, argmin2_tie=True, fp1_is_fp2=False),
              "fp1_last": dict(fp1_last_row=True, fp1_row0=False, argmin1_tie=False, n1_gt_n2=False),
              "fp1_first": dict(fp1_row0=True, fp1_last_row=False, argmin1_tie=False, n1_gt_n2=False)}

# ---------------------------------------------------------------------------------------------------------------------
# 2. the second split of the same leaf: no root, the by-difference path
# ---------------------------------------------------------------------------------------------------------------------


def second_rows(bf, s, kind):
    r"""-> (the m rows of the root split, the m / 2 rows that overflow the X leaf): see the module text.  The Z rows are spread
    among the P rows, the Q row comes in the middle, the last row is a P row."""
    m = bf + 1
    assert m % 2 == 0 and kind in ("le", "gt")
    add = m // 2
    n_q = 1 if kind == "gt" else 0
    n_p = add - s - n_q
    assert n_p >= 1 and m - s - n_q > m // 2 + 1, "the P rows keep the majority"
    kinds = ["P"] * n_p
    for i in range(s):
        kinds.insert((i * len(kinds)) // s, "Z")
    if n_q:
        kinds.insert(len(kinds) // 2, "Q")
    assert kinds[-1] == "P"
    ip = iter(range(m // 2, m))
    later = [camp_row(X_CORE, next(ip), 2) if k == "P" else (Z if k == "Z" else Q) for k in kinds]
    return two_camps(m, m // 2, 2), later, kinds


def second_case(bf, s, kind, n_features=F):
    first, later, _ = second_rows(bf, s, kind)
    return never(bf, n_features), [("packed", rows_of(first, n_features)), ("packed", rows_of(later, n_features))]


# (bf, s, kind): smaller halves of 15, 16, 17, 32 and 33 rows - the engine sums 16 member rows at a time
SECOND = [(127, 15, "le"), (127, 16, "gt"), (127, 17, "le"), (127, 32, "gt"), (127, 33, "le"), (127, 1, "gt")]
# widths: LDS mirror and whole waves (2048), mirror (512, 1024), neither (64, 256, 2056 - a padded row -, 8192)
WIDTHS = [(64, 17, "gt"), (256, 16, "le"), (512, 17, "le"), (1024, 33, "gt"), (2056, 17, "gt"), (8192, 16, "le")]
WIDTH_BF = 127


def second_conditions(s, kind):
    r"""(of the second fit call alone: the X leaf's split)"""
    return dict(splits=True, root=False, internal=False, small_all_single=True, n1_gt_n2=kind == "gt", n1_eq_n2=False, small_over_16=s > 16,
                small_mod16_0=s % 16 == 0, small_mod16_1=s % 16 == 1)


# ---------------------------------------------------------------------------------------------------------------------
# 3. tiers in the node (bbh_tree_fit_buffers, width 4)
# ---------------------------------------------------------------------------------------------------------------------

TIER_BF = 63
# n_samples of the rows of the smaller half (the Z rows), by what the engine's inner loop meets
TIER_NS = {"single": [1] * 18,
           "u8": [1, 2, 255, 1, 1, 200, 1, 3, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1],  # the second group of 16 is uint8 with one-member rows, too
           "u16": [1, 2, 255, 256, 1, 65535, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 300],
           "u32": [1, 2, 255, 256, 65535, 65536, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 70000, 1]}
TIER_CONDITIONS = {"single": dict(small_all_single=True), "u8": dict(small_u8_with_single=True, small_over_255=False),
                   "u16": dict(small_over_255=True, small_over_65535=False), "u32": dict(small_over_65535=True)}


def tier_case(tier, where, last_is_buffer=False):
    r"""where == "leaf": the second split of section 2 (kind "le", s = 18) with TIER_NS[tier] members on the Z rows, through
    bbh_tree_fit_buffers at width 4 (every other row has one member; last_is_buffer: the row that overflows the leaf has 3).
    where == "root": a root of 64 rows that splits 18 : 46 - the Z rows against P rows; it has no tracking row to take a
    difference from and sums both halves."""
    ns_z = TIER_NS[tier]
    s = len(ns_z)
    m = TIER_BF + 1
    if where == "leaf":
        first, later, kinds = second_rows(TIER_BF, s, "le")
        it = iter(ns_z)
        ns = [next(it) if k == "Z" else 1 for k in kinds]
        if last_is_buffer:
            ns[-1] = 3
        ops = [("buffers", features_of(first, [1] * m)), ("buffers", features_of(later, ns))]
    else:
        sets = [camp_row(X_CORE, i, 2) for i in range(m - s)]
        ns = [1] * (m - s)
        for i, n in enumerate(ns_z):
            at = (i * len(sets)) // s
            sets.insert(at, Z)
            ns.insert(at, n)
        if last_is_buffer:
            ns[-1] = 3
        ops = [("buffers", features_of(sets, ns)), ("buffers", features_of([Z, X_CORE + (3, 4), Q], [2, 1, 300]))]
    return never(TIER_BF), ops


TIER_CASES = [(t, w, False) for t in TIER_NS for w in ("root", "leaf")] + [("u8", "leaf", True), ("u16", "root", True)]

# ---------------------------------------------------------------------------------------------------------------------
# 4. natural ties (block rows, diameter 0.5) and internal-node / root splits (lopsided rows, never-merge)
# ---------------------------------------------------------------------------------------------------------------------

NATURAL = [(5, 600), (50, 600), (254, 3000)]  # (bf, rows): bf 254 needs 3 000 rows before a leaf of 255 overflows at all
NATURAL_CONDITIONS = dict(equal_sims_pairs_differ=True, argmin1_tie=True, argmin2_tie=True)


@functools.lru_cache(maxsize=None)
def natural_rows(n):
    return H.block_rows(81, n)


def natural_case(bf, n):
    return T.cfg(bf, 0.5, F, DIAMETER, 0.0, ()), H.cut(natural_rows(n), 3)


@functools.lru_cache(maxsize=None)
def lopsided_rows(n, every, seed=91):
    r"""A common core of 20 eight-bit blocks and one varying block of the next 60; every `every`-th row is an outlier: three
    blocks of its own among the last 176, which no other row of the same stretch shares."""
    rng = np.random.default_rng(seed)
    on = np.zeros((n, 256), bool)
    for i in range(n):
        if i % every == every - 1:
            on[i, 80 + rng.permutation(176)[:3]] = True
        else:
            on[i, :20] = True
            on[i, 20 + rng.integers(0, 60)] = True
    return np.ascontiguousarray(np.packbits(np.repeat(on, 8, axis=1), axis=1))


LOPSIDED = [(3, 600, 3), (50, 600, 2), (254, 5000, 2)]  # (bf, rows, every)
# (at bf 254 these rows split leaves 95 times, lopsidedly, but 5 000 of them make fewer than 255 leaves: the root stays the
# only internal node and never splits again.  The peel rows below reach what that case was meant to.)
LOPSIDED_CONDITIONS = {3: dict(internal=True, root=True, fp1_is_fp2=True), 50: dict(internal=True, root=True), 254: dict(root=True, small_over_16=True)}


@functools.lru_cache(maxsize=None)
def peel_rows(n, seed=93):
    r"""A common core of 160 bits and ONE bit of its own per row.  In a node of such rows every row is 160/161 from the majority
    centroid (the core), fp1 is row 0, every other row is 160/162 from it, fp2 is row 1 and every row but those two is equally
    far from both: only fp1 leaves (n1 = 1), and the next row goes to the rest, which overflows again.  Every row behind the
    first bf + 1 makes a leaf, the nodes above fill with tracking rows of the same kind and split the same way."""
    assert n <= F - 160
    rng = np.random.default_rng(seed)
    pos = rng.permutation(F)
    bits = np.zeros((n, F), bool)
    bits[:, pos[:160]] = True
    bits[np.arange(n), pos[160:160 + n]] = True
    return np.ascontiguousarray(np.packbits(bits, axis=1))


PEEL = [(254, 800)]  # the root fills with 255 tracking rows after 508 rows and splits; the node under it splits again after 254 more
PEEL_CONDITIONS = dict(internal=True, root=True, equal_sims=True, argmin1_tie=True, argmin2_tie=True, m_over_124=True)


def peel_case(bf, n):
    return never(bf), H.cut(peel_rows(n), 3)


def lopsided_case(bf, n, every):
    return never(bf), H.cut(lopsided_rows(n, every), 3)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the three insertion kernels at bf 50 and 254, 2048 bits, diameter criterion at PF.THR
# ---------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def core_families(n, seed=119, runs=()):
    r"""n rows over a common core of 300 bits with 300 bits of their own each (Tanimoto 1/3 with each other: none merges, the
    core keeps them on one path and their leaf splits again and again), each followed by a near-duplicate of an earlier row
    every fourth row (three bits toggled: it merges where the splits left its original on its path).  runs: (row, copies) -
    that many exact copies of a row behind it: BitFeatures of 2 .. 255 members (uint8 sums) and of more (uint16)."""
    rng = np.random.default_rng(seed)
    core = np.zeros(F, bool)
    core[rng.permutation(F)[:300]] = True
    rest = np.flatnonzero(~core)
    out, orig = [], []
    copies = dict(runs)
    for i in range(n):
        row = core.copy()
        row[rng.permutation(rest)[:300]] = True
        orig.append(row)
        out.append(row)
        out += [row] * copies.get(i, 0)
        if i % 4 == 3:
            dup = orig[int(rng.integers(0, len(orig)))].copy()
            dup[rng.integers(0, F, 3)] ^= True
            out.append(dup)
    return np.ascontiguousarray(np.packbits(np.array(out), axis=1))


TAIL_ROWS = {50: 300, 254: 900}  # original rows of a family tail: enough for its leaf to split more than once
# (the seed of the family tail: the first from 95 on with which, in a tree of its own at bf 50, one split has a smaller half of
# s % 16 == 0 rows and another of s % 16 == 1 - the oracle's counters, test_tree_split_cases.py)
TIER_RUNS = ((5, 1), (9, 254), (17, 300), (30, 3), (41, 255), (60, 256), (77, 2))


def zero_tail(bf, seed=99):
    r"""Three all-zero rows (they merge: one BitFeature, row 0 of the root), a family over core A (Tanimoto 1/3 with each other,
    none merges) that overflows the root - the zero row is furthest from the majority centroid and from itself (0 / max(0, 1)):
    fp1 == fp2 == row 0, it leaves alone - and its leaf again, then a family over a core B disjoint from A: its rows are 0 from
    both tracking centroids and go to row 0 of the root, the zero row's leaf, until THAT leaf overflows: a leaf split under a
    parent with room, the zero row is row 0, fp1 == fp2 again.  That leaves bf rows of family B in the leaf, and the next row
    has only a third of core B: it goes there (1/6 from the leaf's tracking centroid, 0 from the others), overflows the leaf as its
    LAST row and is fp1, furthest from the majority centroid.  One more zero row at the end."""
    rng = np.random.default_rng(seed)
    pos = rng.permutation(F)
    n = bf + 60
    bits = np.zeros((3 + 2 * n + 1, F), bool)
    for i in range(2 * n):
        bits[3 + i, pos[:300] if i < n else pos[300:600]] = True
        bits[3 + i, pos[(600 if i < n else 1324) + rng.permutation(724)[:300]]] = True  # (the families share no bit at all)
    bits[3 + n + bf, pos[400:600]] = False
    return np.ascontiguousarray(np.packbits(bits, axis=1))


@functools.lru_cache(maxsize=None)
def tail(name, bf):
    if name == "zeros":
        return zero_tail(bf)
    if name == "blocks":
        # block rows on the last 24 blocks behind a common core (blocks 0..3 set, 4..7 clear): the core keeps them on one path
        # of a tree that holds other rows already, where block rows alone scatter over its leaves
        # (in front of them plain block rows: in a tree of their own THEY are the ones whose leaves split on ties)
        rows = H.block_rows(83, 600 if bf == 50 else 3000, n_features=F - 512)
        core = np.zeros((rows.shape[0], 64), np.uint8)
        core[:, :32] = 0xFF
        return np.ascontiguousarray(np.concatenate([H.block_rows(85, 600 if bf == 50 else 1500), np.concatenate([core, rows], axis=1)]))
    if name == "families":
        return core_families(TAIL_ROWS[bf])
    assert name == "tiers"
    return core_families(TAIL_ROWS[bf], 97, TIER_RUNS)


TAILS = ("blocks", "families", "tiers", "zeros")
KERNEL_CASES = [(name, bf) for bf in (50, 254) for name in TAILS]
KERNEL_CONDITIONS = {"blocks": dict(splits=True, argmin2_tie=True, equal_sims_pairs_differ=True), "families": dict(splits=True), "tiers": dict(splits=True, small_over_255=True), "zeros": dict(splits=True)}
# what a tail must meet in a tree of its own on top of that (the zero row is row 0 of a leaf under a parent with room)
ALONE_CONDITIONS = {"zeros": dict(zero_row=True, fp1_is_fp2=True, fp1_last_row=True)}


def kernel_case(name, bf, prefixed):
    r"""prefixed: behind pipe_forward_cases.prefix(), whose 9 692 rows hand the tree to the pipelined kernel."""
    ops = H.cut(tail(name, bf), 2)
    if prefixed:
        ops = [("packed", PF.prefix())] + ops
    return T.cfg(bf, PF.THR, F, DIAMETER, 0.0, ()), ops


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue: name -> (builder, arguments, (scope, conditions)); what the complete engine runs in-process.  conditions:
# split counter -> True (some split met it) or False (none did), over the splits of the first fit call, of the last one, or of all
# ---------------------------------------------------------------------------------------------------------------------


def _catalogue():
    cat = {}
    for bf in CAMP_BF:
        m = bf + 1
        cat[f"camps-bf{bf}-tie"] = (camps_case, (bf, m // 2), ("first", TIE))
        cat[f"camps-bf{bf}-one-less"] = (camps_case, (bf, m // 2 - 1), ("first", NO_TIE))
        cat[f"camps3-bf{bf}-tie"] = (camps3_case, (bf, m // 2), ("first", TIE3))
        if m > 4:  # (of four rows with one in X, two share another camp: a tie again)
            cat[f"camps3-bf{bf}-one-less"] = (camps3_case, (bf, m // 2 - 1), ("first", NO_TIE))
    for bf in ODD_BF:
        cat[f"camps-bf{bf}-floor"] = (camps_case, (bf, (bf + 1) // 2), ("first", NO_TIE))
        cat[f"camps-bf{bf}-ceil"] = (camps_case, (bf, (bf + 2) // 2), ("first", NO_TIE))
    for kind, cond in NODE_KINDS.items():
        cat[f"node-{kind}"] = (node_case, (kind,), ("first", cond))
    for bf, s, kind in SECOND:
        cat[f"second-bf{bf}-s{s}-{kind}"] = (second_case, (bf, s, kind), ("last", second_conditions(s, kind)))
    for nf, s, kind in WIDTHS:
        cat[f"width{nf}-s{s}-{kind}"] = (second_case, (WIDTH_BF, s, kind, nf), ("last", second_conditions(s, kind)))
    for tier, where, last in TIER_CASES:
        cat[f"tier-{tier}-{where}" + ("-buffer-last" if last else "")] = (tier_case, (tier, where, last), ("first" if where == "root" else "last", dict(TIER_CONDITIONS[tier], root=where == "root")))
    for bf, n in NATURAL:
        cat[f"natural-bf{bf}"] = (natural_case, (bf, n), ("all", NATURAL_CONDITIONS))
    for bf, n, every in LOPSIDED:
        cat[f"lopsided-bf{bf}"] = (lopsided_case, (bf, n, every), ("all", LOPSIDED_CONDITIONS[bf]))
    for bf, n in PEEL:
        cat[f"peel-bf{bf}"] = (peel_case, (bf, n), ("all", PEEL_CONDITIONS))
    return cat


CASES = _catalogue()


def kernel_id(case):
    return f"{case[0]}-bf{case[1]}"


def build(name):
    fn, args, _ = CASES[name]
    return fn(*args)


def replay_ops(c, ops, keep_ls=True):
    r"""The oracle's replay of a case, fit call by fit call: -> (snapshots, split counts after every call); a snapshot is
    tree_abi_cases.snapshot with out_leaf (of the calls so far) and `walk` (OracleEngine.walk) after that call."""
    eng = T.make_oracle(c)
    snaps, outs, counts = [], [], []
    for op in ops:
        outs.append(T.apply_op(eng, op))
        snap = T.snapshot(eng)
        snap["out_leaf"] = list(outs)
        snap["walk"] = eng.walk()
        if not keep_ls:
            del snap["ls"]  # (the walk holds the leaves' sums, too: 160 MB a copy behind the prefix)
        snaps.append(snap)
        counts.append(eng.split_counts())
    eng.close()
    return snaps, counts


@functools.lru_cache(maxsize=4)
def replay(name):
    return replay_ops(*build(name))


@functools.lru_cache(maxsize=1)
def replay_kernel(name, bf, prefixed):
    return replay_ops(*kernel_case(name, bf, prefixed), keep_ls=False)


def scoped(counts, scope):
    r"""The split counts of the first fit call, of the last one alone, or of all."""
    if scope == "first":
        return counts[0]
    if scope == "last":
        return {k: counts[-1][k] - counts[-2][k] for k in counts[-1]}
    assert scope == "all"
    return counts[-1]


def unmet(counts, scope, conditions):
    r"""-> the conditions a replay does not meet (empty: the case is worth running)."""
    c = scoped(counts, scope)
    return {k: c[k] for k, want in conditions.items() if (c[k] > 0) != want}


@functools.lru_cache(maxsize=None)
def kernel_tail_counts(name, bf, prefixed):
    r"""The split counts of a kernel tail's own fit calls (behind the prefix: without the prefix's splits)."""
    counts = replay_kernel(name, bf, prefixed)[1]
    return {k: counts[-1][k] - (counts[0][k] if prefixed else 0) for k in counts[-1]}
