r"""Cases that put the tree engine's NODE STORAGE on its edges ("Node storage" at the top of bblean_amd/csrc/bb_tree.hip: nodes
in blocks of 4 rows, compactions that seal nodes, thaw_node, tree images that load sealed): pure data and builders, no GPU
and no library but the oracle.  test_tree_storage_cases.py holds every case against the conditions it names, on the C oracle
and its storage model alone (bbo_tree_storage, bbo_tree_thaw_counts); test_hip_tree_storage.py replays the same cases on
libbbhip.so and compares leaves, counters, the whole tree image and bbh_tree_memory after every operation.

Rows come in camps: camp c of C owns F / C bits, the first half of them its core (set in every member), the rest the binary
digits of the member's number.  Members of one camp share a path, camps share no bit.  Under the never-merge criterion every
row is appended, an exact copy of row 0 of a leaf lands in that leaf; under the diameter criterion at threshold 1.0 only exact
copies merge.  A builder runs the operations on the oracle as it goes and takes the rows that aim at a leaf (the first, the
last, a middle one of the chain) from the oracle's walk, so a case is still plain data: a configuration and a list of
operations, with the conditions its replay must meet after named operations.
TEST INFRASTRUCTURE - never imported by the product."""
from __future__ import annotations

import functools

import numpy as np

import pipe_forward_cases as PF
import tree_abi_cases as T
import tree_split_cases as S
from tree_abi_cases import DIAMETER, NEVER

NG = 4


def node_blocks(rows):
    return (rows + NG - 1) // NG


def never(bf, F):
    return T.cfg(bf, 0.5, F, NEVER, 0.0, ())


def copies_merge(bf, F):
    return T.cfg(bf, 1.0, F, DIAMETER, 0.0, ())


def camp_row(F, C, c, i):
    r"""Member i of camp c of C, as bits."""
    w = F // C
    core = w // 2
    bits = np.zeros(F, bool)
    bits[c * w:c * w + core] = True
    for j in range(min(w - core, 30)):
        if (i >> j) & 1:
            bits[c * w + core + j] = True
    return bits


def camp_rows(F, C, n, first=1):
    r"""n packed rows, camps in turn, members first, first + 1, ... of each."""
    return np.ascontiguousarray(np.packbits(np.array([camp_row(F, C, k % C, first + k // C) for k in range(n)]), axis=1))


def one_row(F, C, c, i, copies=1):
    return np.ascontiguousarray(np.repeat(np.packbits(camp_row(F, C, c, i))[None, :], copies, axis=0))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle driver: everything observable after EVERY operation, the storage model included
# ---------------------------------------------------------------------------------------------------------------------


def observe(eng, outs, keep_ls=True):
    snap = T.snapshot(eng)
    snap["out_leaf"] = [o for o in outs if isinstance(o, np.ndarray)]
    snap["walk"] = eng.walk()
    snap["storage"] = eng.storage()
    snap["thaw"] = eng.thaw_counts()
    nodes = snap["walk"]["nodes"]
    snap["depth"] = int(nodes[:, 0].max()) if len(nodes) else 1
    if not keep_ls:
        del snap["ls"]
    return snap


def replay_ops(c, ops, keep_ls=True):
    r"""-> the oracle's snapshot after every operation: tree_abi_cases.snapshot with out_leaf (of the fits so far), `walk`,
    `storage` and `thaw` (the model's counters) and `depth`."""
    eng = T.make_oracle(c)
    snaps, outs = [], []
    for op in ops:
        outs.append(T.apply_op(eng, op))
        snaps.append(observe(eng, outs, keep_ls))
    eng.close()
    return snaps


def numbers(snaps, i):
    r"""What the conditions speak of after operation i: the storage model's values and the depth by name, and `+name`: the change
    of a storage value or thaw counter over that operation."""
    cur = dict(snaps[i]["storage"], depth=snaps[i]["depth"], **snaps[i]["thaw"])
    if i > 0:
        old = dict(snaps[i - 1]["storage"], depth=snaps[i - 1]["depth"], **snaps[i - 1]["thaw"])
    else:
        old = {k: 0 for k in cur}
    out = dict(cur)
    for k in cur:
        out["+" + k] = cur[k] - old[k]
    return out


def unmet(snaps, checks):
    r"""-> the conditions a replay does not meet (empty: the case is worth running).  checks: [(operation, {name: wanted})],
    wanted an integer, ">0" or a function of the numbers."""
    bad = []
    for i, cond in checks:
        num = numbers(snaps, i)
        for k, want in cond.items():
            if callable(want):
                want = want(num)
            if (num[k] > 0) if want == ">0" else (num[k] == want):
                continue
            bad.append((i, k, num[k], want))
    return bad


class Builder:
    r"""Runs the operations on the oracle while the case is put together."""

    def __init__(self, c):
        self.c, self.eng, self.ops, self.checks = c, T.make_oracle(c), [], []

    def op(self, *op, **expect):
        self.ops.append(op)
        T.apply_op(self.eng, op)
        if expect:
            self.expect(**expect)

    def expect(self, **cond):
        self.checks.append((len(self.ops) - 1, {("+" + k[2:] if k.startswith("d_") else k): v for k, v in cond.items()}))

    def fit(self, rows, **expect):
        self.op("packed", np.ascontiguousarray(rows), **expect)

    def seal(self, how="compact"):
        r"""Two sealing compactions - the first records the lengths, the second seals what kept its length - or a reload."""
        if how == "reload":
            self.op("reload", runs=0, cold=0, sealed_now=">0")
        else:
            self.op("compact", 1)
            self.op("compact", 1, cold=lambda n: n["live"] - 1, full=1)

    def leaves(self):
        r"""-> [(length, rows (length, F / 8))] of the leaves in chain order."""
        w = self.eng.walk()
        start = np.concatenate([[0], np.cumsum(w["nodes"][:, 2])])
        out = {}
        for k, (_, leaf, ln, pos) in enumerate(w["nodes"].tolist()):
            if leaf:
                out[pos] = (ln, w["cent"][start[k]:start[k] + ln].copy())
        return [out[p] for p in range(len(out))]

    def row_into(self, pos):
        r"""A row of the leaf at chain position `pos` whose exact copy comes back to that leaf (tried on a replay of the
        operations so far: the tracking rows above decide, not the leaf)."""
        ln, rows = self.leaves()[pos]
        return self.row_landing(pos, [rows[r:r + 1] for r in range(ln)])

    def row_landing(self, pos, candidates):
        r"""The first of the candidate rows that ends in the leaf at chain position `pos`."""
        for row in candidates:
            probe = T.make_oracle(self.c)
            for op in self.ops:
                T.apply_op(probe, op)
            hit = int(probe.fit_packed(row)[0])
            w = probe.walk()
            probe.close()
            start = np.concatenate([[0], np.cumsum(w["nodes"][:, 2])])
            k = int(np.searchsorted(start, int(np.flatnonzero((w["id"] == hit))[0]), side="right")) - 1
            if w["nodes"][k, 3] == pos and len(w["nodes"]) == len(self.eng.walk()["nodes"]):  # (and splits nothing)
                return row
        raise AssertionError(f"no candidate row ends in leaf {pos}")

    def path_lengths(self):
        r"""Lengths of the nodes on the path through row 0 of every level."""
        nodes = self.eng.walk()["nodes"]
        depth = int(nodes[:, 0].max())
        return nodes[:depth, 2].tolist()

    def done(self):
        self.eng.close()
        return self.c, self.ops, self.checks


# ---------------------------------------------------------------------------------------------------------------------
# 1. the complete engine
# ---------------------------------------------------------------------------------------------------------------------

# (bf, n_features, camps, rows of a three-level tree): row pieces of RB = 16, 272 and 1024 bytes; bf 3 has one block a node
SHAPES = [(3, 8, 2, 40), (5, 24, 2, 60), (8, 64, 4, 200), (5, 2056, 4, 70), (8, 8192, 4, 200)]


# (at bf 8 a node has 9 rows, three blocks, and every length up to 8 rounds up to fewer: every node but the root is sealed)
LINK_SHAPES = [(8, 64, 4, 96), (8, 2056, 4, 96), (8, 8192, 4, 96)]


def seal_all(bf, F, C, n):
    r"""A three-level tree; compact(1) records and seals nothing, the second seals every node but the root, compact(0) brings all
    back, compact(1) straight after it seals everything again (k_gc_move always records); then rows that thaw."""
    b = Builder(never(bf, F))
    small = ">0" if bf > 3 else 0  # (one block a node at bf 3: a cold node has all the capacity there is)
    b.fit(camp_rows(F, C, n), depth=lambda num: max(num["depth"], 3), thaws=0)
    b.op("compact", 1, runs=1, cold=0, sealed_now=0, full=lambda num: num["live"])
    b.op("compact", 1, runs=2, cold=lambda num: num["live"] - 1, full=1, sealed_now=small)
    b.op("compact", 0, runs=3, cold=0, sealed_now=0, used_blocks=lambda num: num["live"] * node_blocks(bf + 1))
    b.op("compact", 1, runs=4, cold=lambda num: num["live"] - 1, sealed_now=small)
    b.fit(camp_rows(F, C, 2 * C, first=n // C + 2), d_thaws=small)
    b.op("compact", 0, cold=0, sealed_now=0)
    return b.done()


def thaw_links(bf, F, C, n, merge, how, again=True):
    r"""One-element fits after sealing: a copy of row 0 of the first leaf of the chain (its parent is sealed, too: two thaws in
    one descent), of the last leaf, of a middle one (both neighbours are re-pointed), of the first again (nothing is sealed on
    that path any more).  merge: copies merge (no length changes), else they are appended.  Then the holes go (compact(1)),
    the same rows again, and compact(0)."""
    b = Builder(copies_merge(bf, F) if merge else never(bf, F))
    rows = camp_rows(F, C, n)
    # (camp after camp: the leaves of the chain's two ends then hold rows of one camp and their copies come back to them)
    b.fit(rows[np.argsort(np.arange(n) % C, kind="stable")], depth=lambda num: max(num["depth"], 3))
    b.seal(how)
    after = dict(d_then_merge=1, d_then_append=0) if merge else dict(d_then_merge=0, d_then_append=1)
    n_leaves = len(b.leaves())
    rows = [b.row_into(0)]
    b.fit(rows[0], d_first_leaf=1, d_parent_thawed_too=1, d_thaws=lambda num: num["depth"] - 1, **after)
    rows.append(b.row_into(n_leaves - 1))
    b.fit(rows[1], d_last_leaf=1, d_leaf=1, **after)
    for mid in range(n_leaves // 2, n_leaves - 1):  # a middle leaf that is still sealed and that its own rows come back to
        try:
            rows.append(b.row_into(mid))
        except AssertionError:
            continue
        break
    b.fit(rows[2], d_middle_leaf=1, d_leaf=1, **after)
    b.fit(rows[0], d_thaws=0)
    if again:
        b.op("compact", 1, d_used_blocks=lambda num: min(num["+used_blocks"], -1))  # (the holes the thaws left are gone)
        b.fit(np.concatenate(rows), d_thaws=0)  # (a thawed node has no record: one compaction does not seal it again)
        b.op("compact", 0, cold=0, sealed_now=0)
    return b.done()


def length_class(bf, F, L):
    r"""Two camps, a root over two leaves; copies bring one leaf to length L; sealing; one more copy.  A leaf whose length rounds
    up to fewer blocks than bf + 1 rows need is sealed and the copy costs a thaw - with L % 4 == 0 there is no spare row and
    an append without the thaw would land in row 0 of the node behind it; one whose length rounds up to full capacity is
    cold but not sealed and the copy costs none."""
    b = Builder(never(bf, F))
    b.fit(camp_rows(F, 2, bf + 1), depth=2)
    lv = b.leaves()
    at = min(range(len(lv)), key=lambda p: lv[p][0])
    ln, rows = lv[at]
    assert ln <= L, (ln, L)
    if L > ln:
        b.fit(np.repeat(rows[:1], L - ln, axis=0))
    assert b.leaves()[at][0] == L, (b.leaves()[at][0], L)
    b.seal()
    if node_blocks(L) < node_blocks(bf + 1):
        cond = {"d_thaws": 1, "d_append_len%d" % (L % 4): 1, "d_used_blocks": node_blocks(bf + 1) * (2 if L == bf else 1)}
    else:
        cond = dict(d_thaws=0, d_cold_but_full=1)
    b.fit(rows[:1], **cond)
    b.fit(rows[:1], d_thaws=0)
    b.op("compact", 0, cold=0)
    return b.done()


# (bf, n_features, L): every residue of the length mod 4 at bf 8 (rows = 9: three blocks; 8 is a full leaf, the append splits
# it), and the lengths on either side of "rounds up to full capacity" at bf 50, 254 and 1023
LENGTHS = [(8, 64, 4), (8, 64, 5), (8, 24, 6), (8, 64, 7), (8, 2056, 8), (50, 2056, 48), (50, 2056, 49), (254, 64, 252), (254, 64, 253),
           (1023, 64, 1020), (1023, 64, 1021)]


def thaw_then_split(how, F=64):
    r"""bf 8, never-merge, one row over and over: a node of equal rows splits 1 : 8 (fp1 == fp2 == row 0 leaves alone) and every
    copy goes down row 0, so full nodes pile up.  Rows until the root, its row-0 child and that one's row-0 leaf hold 8 rows
    each; sealing; one more: thaw and split of the leaf, thaw and split of its parent, split of the root, a new root."""
    b = Builder(never(8, F))
    row = one_row(F, 2, 0, 1)
    probe = T.make_oracle(b.c)
    n = 0
    while True:
        probe.fit_packed(row)
        n += 1
        nodes = probe.walk()["nodes"]
        if int(nodes[:, 0].max()) == 3 and nodes[:3, 2].tolist() == [8, 8, 8]:
            break
        assert n < 5000
    probe.close()
    b.fit(np.repeat(row, n, axis=0), depth=3)
    assert b.path_lengths() == [8, 8, 8]
    b.seal(how)
    b.fit(row, depth=4, d_thaws=2, d_leaf_then_split=1, d_internal_then_split=1, d_then_new_root=1, d_whole_path_new_root=1,
          d_used_blocks=(2 + 4) * node_blocks(9))
    b.fit(np.repeat(row, 3, axis=0))
    b.op("compact", 0, cold=0)
    return b.done()


def seal_rule():
    r"""What the second of two sealing compactions seals.  bf 8.  After the first: a leaf that gains a row, a leaf that only takes a
    merge (its length stays, its row and the tracking row above change), and a leaf of 8 equal rows that takes a ninth and
    splits 1 : 8 - the half that stays in place has exactly the recorded length, and split_node rewrites only the length
    word, so the record survives.  The second compaction seals the last two and not the first."""
    F, C = 64, 4
    b = Builder(never(8, F))
    b.fit(np.concatenate([one_row(F, C, 0, 1, 16), camp_rows(F, C, 40, first=1)]), depth=2, live=9)
    lv = b.leaves()
    full = [p for p, (ln, rows) in enumerate(lv) if ln == 8 and (rows == rows[0]).all()]
    other = [p for p, (ln, rows) in enumerate(lv) if ln < 8 and not (rows == one_row(F, C, 0, 1)[0]).all(axis=1).any()]
    assert full and len(other) >= 2, (full, other, [ln for ln, _ in lv])
    b.op("compact", 1, cold=0)
    b.op("set_merge", DIAMETER, 0.0, (), 1.0, 8)
    b.fit(lv[other[0]][1][:1], d_then_merge=0, d_thaws=0)  # merges: stats say so below
    b.op("set_merge", NEVER, 0.0, (), 0.5, 8)
    b.fit(lv[other[1]][1][:1])                              # appended: the leaf gains a row
    # the ninth copy splits its leaf 1 : 8 and the root (8 rows, 9 with the new leaf) 1 : 8 under a new root: two halves that stay
    # in place with the 8 rows the first compaction recorded
    b.fit(lv[full[0]][1][:1], d_in_place_half_keeps_record=2, d_live=3, depth=3)
    # 12 nodes.  Full: the new root, the two new halves, the leaf that gained a row.  Cold: the old root and the split leaf (both
    # changed, both at their recorded length), the leaf that took the merge, the five leaves nothing reached.
    b.op("compact", 1, cold=8, full=4, sealed_now=8, live=12)
    b.fit(lv[full[0]][1][:1])
    b.op("compact", 1)
    b.op("compact", 0, cold=0)
    return b.done()


TIER_CFG = T.cfg(5, 0.6, T.TIER_F)  # (tree_abi_cases.TIER_CFG merges these rows into a single node; at 0.6 they make three levels)


def tiers(width, how):
    r"""The bbh_tree_fit_buffers tables of tree_abi_cases.tier_table: rows of the uint8, uint16 and uint32 cluster-feature tiers in
    nodes that are compacted, sealed and thawed (the walk's linear sums read the slot words)."""
    table, _ = T.tier_table(width)
    cut = 2 * table.shape[0] // 3
    b = Builder(TIER_CFG)
    b.op("buffers", np.ascontiguousarray(table[:cut]))
    b.seal(how)
    b.op("buffers", np.ascontiguousarray(table[cut:]), d_thaws=">0", d_then_merge=">0", d_then_append=">0")
    b.op("compact", 1)
    b.op("buffers", np.ascontiguousarray(table[:40]), d_thaws=">0")
    b.op("compact", 0, cold=0)
    return b.done()


def reset_case():
    r"""Compact, seal, reset (the handle keeps its pools and its compaction counters, the thaw count restarts), fit again."""
    F, C = 64, 4
    b = Builder(never(5, F))
    b.fit(camp_rows(F, C, 60))
    b.seal()
    b.fit(camp_rows(F, C, 8, first=40), d_thaws=">0")
    b.op("reset", thaws=0, runs=2, live=1, used_blocks=node_blocks(6))
    b.op("compact", 1, runs=3, full=1, cold=0)
    b.fit(camp_rows(F, C, 50, first=3), thaws=0)
    b.seal()
    b.fit(camp_rows(F, C, 8, first=60), d_thaws=">0")
    b.op("compact", 0, cold=0)
    return b.done()


MANY_F = 2304  # peel rows need 160 bits and one per row: 2 064 rows


def many_blocks():
    r"""bf 1023 (256 blocks a node) and peel rows (tree_split_cases.peel_rows, here at 2304 bits: a node per row behind the first
    1024): 1 035 nodes, 264 960 used blocks when the first compaction comes - more than the 2^18 waves of k_gc_move's largest
    grid, so its grid-stride loop goes round a second time.  The walk after each compaction shows that every node arrived."""
    rng = np.random.default_rng(95)
    n = 1024 + 1040
    pos = rng.permutation(MANY_F)
    bits = np.zeros((n, MANY_F), bool)
    bits[:, pos[:160]] = True
    bits[np.arange(n), pos[160:160 + n]] = True
    rows = np.ascontiguousarray(np.packbits(bits, axis=1))
    ops = [("packed", rows[:2050]), ("compact", 1), ("compact", 1), ("packed", rows[2050:]), ("compact", 0)]
    over = lambda num: max(num["used_blocks"], (1 << 18) + 1)  # noqa: E731
    checks = [(0, {"used_blocks": over, "live": lambda num: max(num["live"], 1026)}), (1, {"cold": 0, "used_blocks": over}),
              (2, {"cold": lambda num: num["live"] - 1, "sealed_now": ">0"}), (4, {"cold": 0, "used_blocks": over})]
    return never(1023, MANY_F), ops, checks


def _catalogue():
    cat = {}
    for bf, F, C, n in SHAPES:
        cat[f"seal_all-bf{bf}-F{F}"] = (seal_all, (bf, F, C, n))
    for bf, F, C, n in LINK_SHAPES:
        for merge in (False, True):
            cat[f"thaw_links-bf{bf}-F{F}-{'merge' if merge else 'append'}"] = (thaw_links, (bf, F, C, n, merge, "compact"))
    cat["reload-thaw_links-append"] = (thaw_links, (8, 64, 4, 96, False, "reload"))
    cat["reload-thaw_links-merge"] = (thaw_links, (8, 2056, 4, 96, True, "reload"))
    for bf, F, L in LENGTHS:
        cat[f"length-bf{bf}-F{F}-L{L}"] = (length_class, (bf, F, L))
    cat["thaw_then_split"] = (thaw_then_split, ("compact",))
    cat["reload-thaw_then_split"] = (thaw_then_split, ("reload",))
    cat["seal_rule"] = (seal_rule, ())
    for width in (1, 2, 4, 8):
        cat[f"tiers-w{width}"] = (tiers, (width, "compact"))
    cat["reload-tiers-w8"] = (tiers, (8, "reload"))
    cat["reset"] = (reset_case, ())
    cat["many_blocks"] = (many_blocks, ())
    return cat


CASES = _catalogue()


@functools.lru_cache(maxsize=None)
def build(name):
    fn, args = CASES[name]
    return fn(*args)


@functools.lru_cache(maxsize=4)
def replay(name):
    c, ops, _ = build(name)
    return replay_ops(c, ops)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the three insertion kernels at bf 50 and 254, 2048 bits: a first tail, sealing (two compactions or a reload), a second
#    tail.  Behind pipe_forward_cases.prefix() the tree belongs to the pipelined kernel when the second tail comes.
# ---------------------------------------------------------------------------------------------------------------------

# (bf, how the tree is sealed, what is in front of the sealing).  "prefix": pipe_forward_cases.prefix(), a tree whose root is a
# zero level - the single-level instance of the pipelined kernel.  "groups": rows over eight cores, whose tracking rows are
# informative on every level - its multi-level instance (pipe_router_ml), which meets the sealed leaf-parents in fill_slot.
KERNEL_CASES = [(bf, how, "prefix") for bf in (50, 254) for how in ("compact", "reload")] + [(50, how, "groups") for how in ("compact", "reload")]


def kernel_id(case):
    return f"bf{case[0]}-{case[1]}" + ("" if case[2] == "prefix" else "-" + case[2])


# rows of the family tail (tree_split_cases.tail("families", bf)) in front of the sealing: behind the prefix the family's leaf then
# holds 48 (252) rows - sealed without a spare row; 50 (254) rows would round up to full capacity, which is never sealed - so
# that the second tail's family rows thaw it, fill it and split it in the same call
FIRST_TAIL = {50: 61, 254: 316}


@functools.lru_cache(maxsize=None)
def scattered(n=300, seed=131):
    r"""n rows of the prefix with three bits toggled each: they go back to leaves all over the tree and merge or are appended."""
    rng = np.random.default_rng(seed)
    rows = PF.prefix()
    bits = np.unpackbits(rows[rng.permutation(rows.shape[0])[:n]], axis=1)
    for r in range(n):
        bits[r, rng.integers(0, S.F, 3)] ^= 1
    return np.ascontiguousarray(np.packbits(bits, axis=1))


N_GROUPED, GROUPED_FIRST = 10_500, 9_800  # more than the 8 192 elements a tree's first launches give the steady-state kernel


@functools.lru_cache(maxsize=None)
def grouped(n=N_GROUPED, groups=8, seed=141):
    r"""Rows of eight groups in turn: the group's core of 300 bits and 300 bits of the row's own.  No two merge at PF.THR, a
    group's rows share a path, and every tracking row keeps its group's core: no level is a zero level."""
    rng = np.random.default_rng(seed)
    cores = [rng.permutation(S.F)[:300] for _ in range(groups)]
    bits = np.zeros((n, S.F), bool)
    for i in range(n):
        bits[i, cores[i % groups]] = True
        bits[i, rng.permutation(S.F)[:300]] = True
    return np.ascontiguousarray(np.packbits(bits, axis=1))


def kernel_case(bf, how, kind="prefix"):
    r"""kind "prefix": behind pipe_forward_cases.prefix(), whose 9 692 rows make a tree of three levels and hand it to the
    pipelined kernel.  The other two kernels get the same rows: alone the tails build a root over leaves, and the root is
    never sealed.  The second tail: scattered rows (sealed leaves under sealed and, later, under thawed leaf-parents), then
    the rest of the family (its leaf is sealed without a spare row: thaw, fill, split).
    kind "groups": 9 800 grouped rows, the sealing, 700 more: they reach every leaf-parent of the three-level tree."""
    c = T.cfg(bf, PF.THR, S.F, DIAMETER, 0.0, ())
    seal = [("reload",)] if how == "reload" else [("compact", 1), ("compact", 1)]
    if kind == "groups":
        rows = grouped()
        return c, [("packed", np.ascontiguousarray(rows[:GROUPED_FIRST]))] + seal + [("packed", np.ascontiguousarray(rows[GROUPED_FIRST:])), ("compact", 0)]
    family = S.tail("families", bf)
    cut = FIRST_TAIL[bf]
    second = np.concatenate([scattered(), family[cut:]])
    ops = [("packed", PF.prefix()), ("packed", np.ascontiguousarray(family[:cut]))] + seal
    return c, ops + [("packed", np.ascontiguousarray(second)), ("compact", 0)]


def second_fit(case):
    r"""The operation that inserts the second tail: the last but one."""
    return len(kernel_case(*case)[1]) - 2


# what the second tail's thaws must meet, by the model: a sealed leaf-parent, a sealed leaf under a leaf-parent that an earlier
# element of the call thawed, a leaf that is thawed and later split in the same call, an append to a sealed leaf without a
# spare row.  The root's tracking rows over the prefix are all-zero majorities: every row goes down row 0 of the root, so one
# leaf-parent is all a "prefix" tail can reach.  The "groups" rows reach all eight.
KERNEL_CONDITIONS = ("leaf_parent", "leaf_under_thawed_parent", "thawed_leaf_splits", "then_append", "append_len0")


@functools.lru_cache(maxsize=2)
def replay_kernel(bf, how, kind="prefix"):
    return replay_ops(*kernel_case(bf, how, kind), keep_ls=False)


def second_tail(case):
    r"""-> what the model's counters gained over the second tail's fit."""
    snaps = replay_kernel(*case)
    return {k[1:]: v for k, v in numbers(snaps, second_fit(case)).items() if k.startswith("+")}


# ---------------------------------------------------------------------------------------------------------------------
# 3. one bbh_trees_fit_packed call over three trees: one sealed by two compactions, one reloaded, one fresh
# ---------------------------------------------------------------------------------------------------------------------


def _by_camp(F, C, n):
    rows = camp_rows(F, C, n)
    return np.ascontiguousarray(rows[np.argsort(np.arange(n) % C, kind="stable")])


def multi_tree():
    r"""-> [(name, cfg, operations before the call, rows of the call)].  The rows of the call are members the trees have not
    seen: they are appended all over the tree and thaw leaves, leaf-parents and, in the sealed trees, nothing else."""
    return [("sealed", never(8, 64), [("packed", _by_camp(64, 4, 96)), ("compact", 1), ("compact", 1)], camp_rows(64, 4, 24, first=30)),
            ("reloaded", never(8, 2056), [("packed", _by_camp(2056, 4, 96)), ("reload",)], camp_rows(2056, 4, 20, first=40)),
            ("fresh", never(5, 24), [], camp_rows(24, 2, 60))]


@functools.lru_cache(maxsize=None)
def replay_multi_tree():
    r"""name -> the oracle's snapshots of that tree: after every operation before the call, then after the call's rows."""
    return {name: replay_ops(c, before + [("packed", rows)]) for name, c, before, rows in multi_tree()}
