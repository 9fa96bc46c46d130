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

    def u32(self, at: int) -> int:
        return struct.unpack_from("<I", self.buf, at)[0]

    def put_u32(self, at: int, v: int) -> None:
        struct.pack_into("<I", self.buf, at, v)

    def node(self, ib: int) -> dict:
        ln, word, prev, nxt = struct.unpack_from("<4I", self.buf, self.hdr_at(ib))
        return dict(len=ln, leaf=word & 1, cap=word >> 16, prev=prev, next=nxt)

    def live_nodes(self) -> list[int]:
        return [b for b in range(self.T) if self.node(b)["cap"]]


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
