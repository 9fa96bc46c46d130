r"""The tree-image layout (include/bbhip.h "Tree images", bb_tree_image.inc, INTEGRATION.md "Tree files") written down a
second time, in Python, for the persistence tests: a parser that finds every field of a real image, so that a test can
damage exactly one of them, and a hand-built image of a three-node tree, so that the host check can be exercised without a
device.  TEST INFRASTRUCTURE - never imported by the product."""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"BBHTREE\x00"
HEADER_BYTES = 512
GROUP_BLOCKS = 64
NG = 4
NONE = 0xFFFFFFFF
C_NODES, C_IDS, C_N8, C_N16, C_N32, C_ROOT, C_FIRST_LEAF, C_DEPTH = range(8)
_HDR = struct.Struct("<8s4I4i6I8I2d8Q6Q")  # 224 bytes, zero padding up to 512
assert _HDR.size == 224


def row_bytes(n_features: int) -> int:
    return (n_features // 8 + 15) // 16 * 16


def block_bytes(rb: int) -> int:
    return NG * (rb + 40) + 16


def pack_header(**kw) -> bytes:
    h = dict(magic=MAGIC, version=1, endian=0x01020304, header_bytes=HEADER_BYTES, group_blocks=GROUP_BLOCKS, ng=NG)
    h.update(kw)
    vals = [h["magic"], h["version"], h["endian"], h["header_bytes"], h["group_blocks"], h["bf"], h["F"], h["crit"], h["tol_len"],
            h["ng"], h["rb"], h["n_blocks"], h["n8"], h["n16"], h["n32"], *h["ctr"], h["thr"], h["tolerance"], *h["stats"],
            h["tol_bytes"], h["node_bytes"], h["cf8_bytes"], h["cf16_bytes"], h["cf32_bytes"], h["image_bytes"]]
    return _HDR.pack(*vals).ljust(HEADER_BYTES, b"\0")


def parse_header(buf: bytes) -> dict:
    v = _HDR.unpack_from(buf, 0)
    names = ["magic", "version", "endian", "header_bytes", "group_blocks", "bf", "F", "crit", "tol_len", "ng", "rb", "n_blocks", "n8", "n16", "n32"]
    h = dict(zip(names, v[:15]))
    h["ctr"] = list(v[15:23])
    h["thr"], h["tolerance"] = v[23:25]
    h["stats"] = list(v[25:33])
    for k, x in zip(["tol_bytes", "node_bytes", "cf8_bytes", "cf16_bytes", "cf32_bytes", "image_bytes"], v[33:39]):
        h[k] = x
    return h


class Image:
    r"""Byte offsets into an image held in a bytearray (`buf`, the image starts at `base`)."""

    def __init__(self, buf: bytearray, base: int = 0):
        self.buf, self.base = buf, base
        self.h = parse_header(bytes(buf[base:base + HEADER_BYTES]))
        self.T, self.rb = self.h["n_blocks"], self.h["rb"]
        self.nodes_at = base + HEADER_BYTES + self.h["tol_bytes"]
        self.sections = [base + HEADER_BYTES, self.nodes_at]  # where every section after the header begins ... and the end
        for k in ("node_bytes", "cf8_bytes", "cf16_bytes", "cf32_bytes"):
            self.sections.append(self.sections[-1] + self.h[k])

    def _group(self, ib: int) -> tuple[int, int, int]:
        g = ib // GROUP_BLOCKS
        m = min(GROUP_BLOCKS, self.T - g * GROUP_BLOCKS)
        return self.nodes_at + g * GROUP_BLOCKS * block_bytes(self.rb), m, ib % GROUP_BLOCKS

    def hdr_at(self, ib: int) -> int:
        at, _, i = self._group(ib)
        return at + i * 16

    def link_at(self, ib: int, row: int) -> int:
        at, m, i = self._group(ib + row // NG)
        return at + m * 16 + (i * NG + row % NG) * 4

    def rm_at(self, ib: int, row: int) -> int:
        at, m, i = self._group(ib + row // NG)
        return at + m * 32 + (i * NG + row % NG) * 32

    def card_at(self, ib: int, row: int) -> int:
        at, m, i = self._group(ib + row // NG)
        return at + m * 160 + (i * NG + row % NG) * 4

    def cent_at(self, ib: int, row: int) -> int:
        at, m, i = self._group(ib + row // NG)
        return at + m * 176 + (i * NG + row % NG) * self.rb

    def row(self, ib: int, row: int) -> dict:
        r"""The row record of row `row` of the node that starts at block `ib`: BitFeature id, n_samples, slot word."""
        sub, n, slot = struct.unpack_from("<3I", self.buf, self.rm_at(ib, row))
        return dict(sub=sub, n=n, tier=slot >> 30, slot=slot & 0x3FFFFFFF)

    def linear_sum(self, leaf: bool, rec: dict, cent: np.ndarray) -> np.ndarray:
        r"""The linear sum (F uint64) of a row: a leaf row of one member keeps it in its centroid row, every other row in the
        cluster-feature section its slot word names (tier 0 / 1 / 2: cf8 / cf16 / cf32); tracking rows are always cf32."""
        F = self.h["F"]
        if leaf and rec["n"] == 1:
            return np.unpackbits(cent)[:F].astype(np.uint64)
        assert rec["tier"] == 2 if not leaf else rec["tier"] in (0, 1, 2), ("tier", leaf, rec)
        width = 1 << rec["tier"]
        assert rec["slot"] < (self.h["n8"], self.h["n16"], self.h["n32"])[rec["tier"]], ("slot beyond its section", rec)
        at = self.sections[2 + rec["tier"]] + rec["slot"] * F * width
        return np.frombuffer(self.buf, dtype=("<u1", "<u2", "<u4")[rec["tier"]], count=F, offset=at).astype(np.uint64)

    def walk(self) -> dict:
        r"""The whole tree in pre-order - the root (ctr[C_ROOT]) first, then the subtrees of its rows in row order, by their
        link words - in the shape of OracleEngine.walk: nodes (n, 4) int32 [depth (the root is 1), leaf flag, length,
        position in the leaf chain from ctr[C_FIRST_LEAF] or -1], and per row (node after node) n, id, pop, cent, ls."""
        F, nb = self.h["F"], self.h["F"] // 8
        if self.T == 0:
            return dict(nodes=np.empty((0, 4), np.int32), n=np.empty(0, np.uint64), id=np.empty(0, np.uint32), pop=np.empty(0, np.uint32),
                        cent=np.empty((0, nb), np.uint8), ls=np.empty((0, F), np.uint64))
        pos, b, before = {}, self.h["ctr"][C_FIRST_LEAF], NONE
        while b != NONE:
            assert b not in pos and b < self.T, "the leaf chain loops or leaves the image"
            assert self.node(b)["prev"] == before, f"leaf {b} at chain position {len(pos)}: prev is {self.node(b)['prev']}, the leaf before it is {before}"
            pos[b] = len(pos)
            before, b = b, self.node(b)["next"]
        nodes, ns, ids, pops, cents, lss = [], [], [], [], [], []
        seen = set()

        def visit(ib, depth):
            assert ib < self.T and ib not in seen, ("link word", ib)
            seen.add(ib)
            nd = self.node(ib)
            assert nd["cap"] >= nd["len"], ("node header", ib, nd)
            nodes.append([depth, nd["leaf"], nd["len"], pos.get(ib, -1) if nd["leaf"] else -1])
            for r in range(nd["len"]):
                rec = self.row(ib, r)
                cent = np.frombuffer(self.buf, np.uint8, count=nb, offset=self.cent_at(ib, r))
                ns.append(rec["n"])
                ids.append(rec["sub"])
                pops.append(self.u32(self.card_at(ib, r)))
                cents.append(cent)
                lss.append(self.linear_sum(bool(nd["leaf"]), rec, cent))
            if not nd["leaf"]:
                for r in range(nd["len"]):
                    visit(self.u32(self.link_at(ib, r)), depth + 1)

        visit(self.h["ctr"][C_ROOT], 1)
        return dict(nodes=np.array(nodes, np.int32).reshape(-1, 4), n=np.array(ns, np.uint64), id=np.array(ids, np.uint32),
                    pop=np.array(pops, np.uint32), cent=np.array(cents, np.uint8).reshape(-1, nb), ls=np.array(lss, np.uint64).reshape(-1, F))

    def u32(self, at: int) -> int:
        return struct.unpack_from("<I", self.buf, at)[0]

    def put_u32(self, at: int, v: int) -> None:
        struct.pack_into("<I", self.buf, at, v)

    def node(self, ib: int) -> dict:
        ln, word, prev, nxt = struct.unpack_from("<4I", self.buf, self.hdr_at(ib))
        return dict(len=ln, leaf=word & 1, cap=word >> 16, prev=prev, next=nxt)

    def live_nodes(self) -> list[int]:
        return [b for b in range(self.T) if self.node(b)["cap"]]


def walk_children(walk: dict):
    r"""-> (row_start, children): the first row of every node of a walk, and children[k] = the nodes its rows link to (in row
    order; empty for a leaf), from the pre-order alone."""
    nodes = walk["nodes"]
    row_start = np.concatenate([[0], np.cumsum(nodes[:, 2])]).astype(np.int64)
    children = [[] for _ in range(len(nodes))]
    at = 0

    def parse():
        nonlocal at
        k = at
        assert k < len(nodes), "the pre-order ends inside a node's subtrees"
        at += 1
        if not nodes[k, 1]:
            for _ in range(int(nodes[k, 2])):
                c = at
                assert c < len(nodes) and nodes[c, 0] == nodes[k, 0] + 1, f"node {k}: a child is missing or on the wrong level"
                children[k].append(c)
                parse()
        return k

    if len(nodes):
        parse()
    assert at == len(nodes), "nodes beyond the root's subtrees"
    return row_start, children


def walk_faults(walk: dict) -> list[str]:
    r"""What every tree must satisfy, checked on a walk whatever produced it; -> the broken invariants, in words.
    - a tracking row's n_samples and linear sum are the sums over the rows of the node it links to, its id is 0xFFFFFFFF;
    - every row's centroid is bit j = (2 * ls[j] >= n) (n <= 1: ls[j] != 0) and its popcount is that centroid's;
    - leaf rows carry distinct ids; all leaves are on the deepest level;
    - the leaf chain visits every leaf exactly once (positions 0 .. leaves - 1), internal nodes are not on it."""
    faults = []
    nodes = walk["nodes"]
    if len(nodes) == 0:
        return faults
    try:
        row_start, children = walk_children(walk)
    except AssertionError as e:
        return [f"structure: {e}"]
    F = walk["ls"].shape[1]
    n, ls = walk["n"], walk["ls"]
    want = np.where((n <= 1)[:, None], ls != 0, 2 * ls >= n[:, None])
    got = np.unpackbits(walk["cent"], axis=1)[:, :F].astype(bool)
    row_node = np.repeat(np.arange(len(nodes)), nodes[:, 2])
    for r in np.flatnonzero((want != got).any(axis=1))[:5]:
        faults.append(f"row {r - row_start[row_node[r]]} of node {row_node[r]} (n {n[r]}): the centroid is not the majority of its linear sum, "
                      f"first at feature {int(np.argmax(want[r] != got[r]))}")
    if np.unpackbits(walk["cent"], axis=1)[:, F:].any():
        faults.append("a centroid row has bits beyond n_features")
    for r in np.flatnonzero(got.sum(axis=1) != walk["pop"])[:5]:
        faults.append(f"row {r - row_start[row_node[r]]} of node {row_node[r]}: popcount {walk['pop'][r]}, its centroid has {int(got[r].sum())}")
    for k in range(len(nodes)):
        lo, hi = row_start[k], row_start[k + 1]
        if nodes[k, 1]:
            if (walk["id"][lo:hi] == NONE).any():
                faults.append(f"leaf {k}: a row without an id")
            continue
        if (walk["id"][lo:hi] != NONE).any():
            faults.append(f"internal node {k}: a tracking row with an id")
        for j, c in enumerate(children[k]):
            clo, chi = row_start[c], row_start[c + 1]
            if int(n[lo + j]) != int(n[clo:chi].sum()):
                faults.append(f"row {j} of node {k}: n_samples {n[lo + j]}, its child's rows add up to {int(n[clo:chi].sum())}")
            d = ls[lo + j] != ls[clo:chi].sum(axis=0)
            if d.any():
                f = int(np.argmax(d))
                faults.append(f"row {j} of node {k}: linear sum differs from the sum over its child's rows in {int(d.sum())} features, first {f}: "
                              f"{ls[lo + j, f]} against {int(ls[clo:chi, f].sum())}")
    leaf_ids = walk["id"][np.repeat(nodes[:, 1] != 0, nodes[:, 2])]
    if len(set(leaf_ids.tolist())) != leaf_ids.size:
        faults.append("two leaf rows share an id")
    leaves = nodes[nodes[:, 1] != 0]
    if (leaves[:, 0] != nodes[:, 0].max()).any():
        faults.append("a leaf above the deepest level")
    if sorted(leaves[:, 3].tolist()) != list(range(len(leaves))):
        faults.append(f"the leaf chain does not visit every leaf exactly once: positions {sorted(leaves[:, 3].tolist())[:8]}... of {len(leaves)} leaves")
    if (nodes[nodes[:, 1] == 0][:, 3] != -1).any():
        faults.append("an internal node with a chain position")
    return faults


def check_walk(walk: dict, who: str) -> None:
    faults = walk_faults(walk)
    assert not faults, f"{who}: " + "; ".join(faults[:6])


def same_walk(got: dict, want: dict, who: str = "image against oracle") -> None:
    r"""Two walks are equal, exactly: structure, lengths, chain positions and every row's n_samples, id, popcount, centroid and
    linear sum; the message names the first node and row that differ."""
    assert got["nodes"].shape == want["nodes"].shape and (got["nodes"] == want["nodes"]).all(), \
        f"{who}: tree structure [depth, leaf, length, chain position] differs, first at node " \
        f"{int(np.argmax((got['nodes'] != want['nodes']).any(axis=1))) if got['nodes'].shape == want['nodes'].shape else (got['nodes'].shape, want['nodes'].shape)}"
    row_node = np.repeat(np.arange(len(want["nodes"])), want["nodes"][:, 2])
    row_start = np.concatenate([[0], np.cumsum(want["nodes"][:, 2])])
    for key in ("n", "id", "pop", "cent", "ls"):
        a, b = got[key], want[key]
        assert a.shape == b.shape, (who, key, a.shape, b.shape)
        d = (a != b) if a.ndim == 1 else (a != b).any(axis=1)
        if d.any():
            r = int(np.argmax(d))
            k = int(row_node[r])
            kind = "leaf" if want["nodes"][k, 1] else "internal node"
            detail = f"{a[r]} against {b[r]}" if a.ndim == 1 else f"{int((a[r] != b[r]).sum())} entries, first {int(np.argmax(a[r] != b[r]))}: {a[r][np.argmax(a[r] != b[r])]} against {b[r][np.argmax(a[r] != b[r])]}"
            raise AssertionError(f"{who}: `{key}` differs in {int(d.sum())} rows, first row {r - row_start[k]} of node {k} ({kind}, depth {want['nodes'][k, 0]}): {detail}")


def walk_leaves(walk: dict) -> dict:
    r"""The leaf rows of a walk in chain order: what bbh_tree_export_leaves / bbo_tree_export_leaves give."""
    nodes = walk["nodes"]
    row_start = np.concatenate([[0], np.cumsum(nodes[:, 2])]).astype(np.int64)
    order = sorted((int(nodes[k, 3]), k) for k in range(len(nodes)) if nodes[k, 1])
    rows = np.concatenate([np.arange(row_start[k], row_start[k + 1]) for _, k in order]) if order else np.empty(0, np.int64)
    return dict(ids=walk["id"][rows], ns=walk["n"][rows], cents=walk["cent"][rows], ls=walk["ls"][rows])


def synthetic_image(n_features: int = 64, bf: int = 5) -> bytes:
    r"""A valid image built by hand: an internal root (blocks 0-1: bf + 1 = 6 rows) over two leaves (blocks 2 and 3) of two
    one-fingerprint BitFeatures each."""
    assert 4 < bf + 1 <= 8
    rb = row_bytes(n_features)
    T, n8, n16, n32 = 4, 1, 0, 2
    hdr = np.zeros((T, 4), dtype="<u4")
    link = np.zeros((T, NG), dtype="<u4")
    rm = np.zeros((T, NG, 8), dtype="<u4")  # sub, n, slot, pad, s1 (2 words), s2 (2 words)
    card = np.zeros((T, NG), dtype="<u4")
    cent = np.zeros((T, NG, rb), dtype=np.uint8)

    def word(leaf, length, cap):
        return leaf | ((length + 1) << 4) | (cap << 16)

    hdr[0] = [2, word(0, 2, bf + 1), NONE, NONE]
    hdr[2] = [2, word(1, 2, NG), NONE, 3]
    hdr[3] = [2, word(1, 2, NG), 2, NONE]
    link[0, :2] = [2, 3]
    for r in range(2):
        rm[0, r, :3] = [NONE, 2, (2 << 30) | r]
    sub = 0
    for b in (2, 3):
        for r in range(2):
            rm[b, r, :3] = [sub, 1, 0]
            cent[b, r, 0] = 1 << sub
            card[b, r] = 1
            rm[b, r, 4] = rm[b, r, 6] = 1
            sub += 1
    nodes = hdr.tobytes() + link.tobytes() + rm.tobytes() + card.tobytes() + cent.tobytes()
    assert len(nodes) == T * block_bytes(rb)
    cf8 = bytes(n8 * n_features)
    cf32 = np.ones((n32, n_features), dtype="<u4").tobytes()
    ctr = [T, 4, n8, n16, n32, 0, 2, 2]
    stats = [0, 0, 0, 4, 1, 3, 2, 0]
    sizes = dict(tol_bytes=0, node_bytes=len(nodes), cf8_bytes=len(cf8), cf16_bytes=0, cf32_bytes=len(cf32))
    head = pack_header(bf=bf, F=n_features, crit=0, tol_len=0, rb=rb, n_blocks=T, n8=n8, n16=n16, n32=n32, ctr=ctr, thr=0.65,
                       tolerance=0.0, stats=stats, image_bytes=HEADER_BYTES + sum(sizes.values()), **sizes)
    return head + nodes + cf8 + cf32


def damaged(image: bytes, base: int = 0) -> dict[str, bytes]:
    r"""Copies of a valid image (an internal root with at least two leaf children), each with ONE structural fault."""
    out = {}

    def copy():
        return Image(bytearray(image), base)

    im = copy()
    nodes = im.live_nodes()
    root = im.h["ctr"][C_ROOT]
    assert not im.node(root)["leaf"], "the image's root must be an internal node"
    leaves = [b for b in nodes if im.node(b)["leaf"]]
    first = im.h["ctr"][C_FIRST_LEAF]
    im.put_u32(im.link_at(root, 0), im.T + 7)
    out["child link beyond the block count"] = bytes(im.buf)
    im = copy()
    big = next((b for b in nodes if im.node(b)["cap"] > NG), None)  # a node of two blocks and more (the root, unless bf <= 3)
    if big is not None:
        im.put_u32(im.link_at(root, 0), big + 1)
        out["link into the middle of a node"] = bytes(im.buf)
    im = copy()
    im.put_u32(im.rm_at(first, 0) + 8, (1 << 30) | im.h["n16"])  # the first leaf's first row: uint16 slot n16
    out["cluster-feature slot beyond its count"] = bytes(im.buf)
    im = copy()
    im.put_u32(im.rm_at(root, 0) + 8, (2 << 30) | (im.h["n32"] + 3))
    out["tracking slot beyond its count"] = bytes(im.buf)
    for tier in (0, 1, 3):  # the index is fine for the uint32 pool: the kernels would STORE through the tier bits
        im = copy()
        im.put_u32(im.rm_at(root, 0) + 8, (tier << 30) | (im.u32(im.rm_at(root, 0) + 8) & 0x3FFFFFFF))
        out[f"tracking slot with the tier of another pool ({tier})"] = bytes(im.buf)
    im = copy()
    second = im.node(first)["next"]
    assert second != NONE
    im.put_u32(im.hdr_at(second) + 12, first)  # second leaf -> first leaf
    out["leaf chain that loops"] = bytes(im.buf)
    im = copy()
    leaf = leaves[-1]
    im.put_u32(im.hdr_at(leaf), im.node(leaf)["cap"] + 1)
    out["length above capacity"] = bytes(im.buf)
    im = copy()
    struct.pack_into("<I", im.buf, base + 64 + 4 * C_DEPTH, 1)  # ctr[C_DEPTH]
    out["deeper than the recorded depth"] = bytes(im.buf)
    im = copy()
    struct.pack_into("<I", im.buf, base + 64 + 4 * C_DEPTH, im.h["ctr"][C_DEPTH] + 1)
    out["leaves above the recorded depth"] = bytes(im.buf)
    # the insertion kernels take a leaf row's slot from its link word, not from its row record
    for name, word in (("leaf link beyond its tier's count", (2 << 30) | (im.h["n32"] + 1)),
                       ("leaf link far beyond every pool", 0x3FFFFFFF), ("leaf link of no tier", (3 << 30) | 0)):
        im = copy()
        im.put_u32(im.link_at(leaves[-1], 0), word)
        out[name] = bytes(im.buf)
    im = copy()
    inner = next((b for b in nodes if not im.node(b)["leaf"] and b != root), root)
    im.put_u32(im.hdr_at(inner), 0)  # an internal node of length 0 (its children then hang off nothing, too)
    out["internal node without children"] = bytes(im.buf)
    return out
