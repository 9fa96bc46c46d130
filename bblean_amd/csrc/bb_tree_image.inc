// bb_tree_image.inc -- tree images: one fitted tree as a self-contained, relocatable byte stream (bbh_tree_save_fd,
// bbh_tree_load_fd, bbh_tree_image_check_fd; DESIGN.md section 5c, INTEGRATION.md "Tree files").  Included at the end of
// bb_tree.hip.
//
// Layout (version 1, little-endian, every section follows the previous one without padding):
//   header     512 bytes, ImgHeader below
//   tolerance  tol_len float64
//   nodes      n_blocks blocks of NG rows in GROUPS of IMG_GB blocks (the last group holds what is left, m blocks):
//                NodeHdr[m] | link uint32[m * NG] | RowMeta[m * NG] | card uint32[m * NG] | centroid rows[m * NG][RB]
//              i.e. block_bytes() per block, and what the structural check reads (headers, links, row records) comes first.
//   cf8        n8  x F uint8      the used prefixes of the cluster-feature pools: slot numbers stay valid
//   cf16       n16 x F uint16
//   cf32       n32 x F uint32
// In the image every node but the root has the capacity of a sealed node (its length rounded up to a block of rows, "Node
// storage" at the top of bb_tree.hip), the root bf + 1 rows; ids are image block numbers; rows beyond a node's length and
// the headers of blocks that start no node are zero.  A tree that never received anything has n_blocks == 0 and no pools.
//
// Export does not go through gc_nodes: that would need a second copy of the pools in HBM and would renumber the live tree.
// It borrows the compaction's two passes instead - k_img_size + exclusive scan = image ids, k_img_pack = k_gc_move into a
// STAGING buffer for a range of image groups at a time - and leaves the live tree untouched.

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>

namespace {

constexpr uint32_t IMG_GB = 64;  // blocks per group: the unit of staging (smallest stage_bytes = one group)
constexpr uint32_t IMG_VERSION = 1;
constexpr uint32_t IMG_ENDIAN = 0x01020304u;
constexpr uint64_t IMG_DEFAULT_STAGE = 64ull << 20;  // stage_bytes == 0: the size of a streaming-ingest slab (HostSlabs)
const char IMG_MAGIC[8] = {'B', 'B', 'H', 'T', 'R', 'E', 'E', '\0'};

struct ImgHeader {
    char magic[8];
    uint32_t version, endian, header_bytes, group_blocks;
    int32_t bf, F, crit, tol_len;
    uint32_t ng, rb, n_blocks, n8, n16, n32;  // n8 / n16 / n32: slots in the cluster-feature sections
    uint32_t ctr[C_COUNT];                    // the tree's counters, node ids as image block numbers
    double thr, tolerance;
    uint64_t stats[8];
    uint64_t tol_bytes, node_bytes, cf8_bytes, cf16_bytes, cf32_bytes, image_bytes;
    uint8_t pad[512 - 224];
};
static_assert(sizeof(ImgHeader) == 512 && C_COUNT == 8, "tree image header layout");

__host__ __device__ inline size_t img_block_bytes(uint32_t RB) { return (size_t)NG * ((size_t)RB + 40) + sizeof(NodeHdr); }

// where image block `ib` lies in a buffer that starts at group `g0` and holds whole groups in file layout
struct ImgSlot {
    size_t base;      // byte offset of the block's group
    uint32_t m, idx;  // blocks in that group, the block's index in it
    __host__ __device__ size_t hdr() const { return base + (size_t)idx * 16; }
    __host__ __device__ size_t link(uint32_t j) const { return base + (size_t)m * 16 + ((size_t)idx * NG + j) * 4; }
    __host__ __device__ size_t rm(uint32_t j) const { return base + (size_t)m * 32 + ((size_t)idx * NG + j) * 32; }
    __host__ __device__ size_t card(uint32_t j) const { return base + (size_t)m * 160 + ((size_t)idx * NG + j) * 4; }
    __host__ __device__ size_t cent(uint32_t j, uint32_t RB) const { return base + (size_t)m * 176 + ((size_t)idx * NG + j) * (size_t)RB; }
};
static_assert(NG == 4 && sizeof(RowMeta) == 32 && sizeof(NodeHdr) == 16, "tree image group layout");
__host__ __device__ inline ImgSlot img_slot(uint32_t ib, uint32_t g0, uint32_t T, uint32_t RB) {
    const uint32_t g = ib / IMG_GB;
    ImgSlot s;
    s.base = (size_t)(g - g0) * IMG_GB * img_block_bytes(RB);
    s.m = T - g * IMG_GB < IMG_GB ? T - g * IMG_GB : IMG_GB;
    s.idx = ib % IMG_GB;
    return s;
}

// Pass 1 (k_gc_size's twin), one thread per block of the used part of the pool: blocks of the node that starts here in the
// image - 0 for a block that starts no live node, bf + 1 rows for the root, the length rounded up to a block otherwise.
__global__ __launch_bounds__(256) void k_img_size(const NodeHdr* __restrict__ hdr, uint32_t used, uint32_t rows, uint32_t root,
                                                  uint32_t* __restrict__ sz) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= used) return;
    const NodeHdr h = hdr[b];
    uint32_t blocks = 0;
    if (hw_cap(h.leaf) != 0) blocks = b == root ? node_blocks(rows) : node_blocks(h.len > 0 ? h.len : 1u);
    sz[b] = blocks;
}

// Pass 2 (k_gc_move's twin, after the exclusive prefix sum of the sizes = the image ids), one wave per live node: the part
// of the image blocks [lo, hi) - whole groups, `stage` starts at group lo / IMG_GB and was zeroed - that the node covers
// is written in file layout; child ids and the leaf chain's ids are translated.  Nothing of the source tree is written.
// `newid` holds used + 1 entries and does not decrease: a binary search finds the first node that reaches into the range.
__global__ __launch_bounds__(256) void k_img_pack(TreeDev t, uint32_t used, uint32_t rows, const uint32_t* __restrict__ sz,
                                                  const uint32_t* __restrict__ newid, uint32_t T, uint32_t lo, uint32_t hi,
                                                  uint8_t* __restrict__ stage) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * 4u;
    uint32_t a = 0, z = used;
    while (a < z) {
        const uint32_t mid = a + (z - a) / 2;
        if (newid[mid + 1] > lo) z = mid; else a = mid + 1;
    }
    const uint32_t RB = (uint32_t)t.RB, rbc = RB / 16, g0 = lo / IMG_GB;
    for (uint32_t b = a + blockIdx.x * 4u + (threadIdx.x >> 6); b < used; b += waves) {
        const uint32_t nb = newid[b];
        if (nb >= hi) break;
        const uint32_t blocks = sz[b];
        if (blocks == 0) continue;
        const NodeHdr h = t.node_hdr[b];
        const uint32_t len = h.len < blocks * NG ? h.len : blocks * NG;
        const bool leaf = (h.leaf & HW_LEAF) != 0;
        const size_t so = (size_t)b * NG;
        for (uint32_t r = lane; r < len; r += 64) {
            const uint32_t ib = nb + r / NG;
            if (ib < lo || ib >= hi) continue;
            const ImgSlot s = img_slot(ib, g0, T, RB);
            const uint32_t lk = t.node_link[so + r];
            *(uint32_t*)(stage + s.link(r % NG)) = leaf ? lk : (lk < used ? newid[lk] : lk);
            *(RowMeta*)(stage + s.rm(r % NG)) = t.node_rm[so + r];
            *(uint32_t*)(stage + s.card(r % NG)) = t.node_card[so + r];
        }
        const uint4* src = (const uint4*)(t.node_cent + so * (size_t)RB);
        for (uint32_t i = lane; i < len * rbc; i += 64) {
            const uint32_t r = i / rbc, ib = nb + r / NG;
            if (ib < lo || ib >= hi) continue;
            const ImgSlot s = img_slot(ib, g0, T, RB);
            *(uint4*)(stage + s.cent(r % NG, RB) + (size_t)(i % rbc) * 16) = src[i];
        }
        if (lane == 0 && nb >= lo) {
            NodeHdr hn;
            hn.len = len;
            const uint32_t cap = blocks == node_blocks(rows) ? rows : blocks * NG;
            hn.leaf = (h.leaf & HW_LEAF) | (((len + 1) & 0xFFFu) << 4) | (cap << 16);
            hn.prev = (h.prev != NONE && h.prev < used) ? newid[h.prev] : NONE;
            hn.next = (h.next != NONE && h.next < used) ? newid[h.next] : NONE;
            *(NodeHdr*)(stage + img_slot(nb, g0, T, RB).hdr()) = hn;
        }
    }
}

// Import: the image blocks [lo, hi) from a staging buffer in file layout into the node pools, one wave per block.
__global__ __launch_bounds__(256) void k_img_unpack(TreeDev t, uint32_t T, uint32_t lo, uint32_t hi, const uint8_t* __restrict__ stage) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * 4u;
    const uint32_t RB = (uint32_t)t.RB, rbc = RB / 16, g0 = lo / IMG_GB;
    for (uint32_t ib = lo + blockIdx.x * 4u + (threadIdx.x >> 6); ib < hi; ib += waves) {
        const ImgSlot s = img_slot(ib, g0, T, RB);
        const size_t dn = (size_t)ib * NG;
        if (lane == 0) t.node_hdr[ib] = *(const NodeHdr*)(stage + s.hdr());
        if (lane < NG) {
            t.node_link[dn + lane] = *(const uint32_t*)(stage + s.link(lane));
            t.node_rm[dn + lane] = *(const RowMeta*)(stage + s.rm(lane));
            t.node_card[dn + lane] = *(const uint32_t*)(stage + s.card(lane));
        }
        uint4* dst = (uint4*)(t.node_cent + dn * (size_t)RB);
        for (uint32_t i = lane; i < NG * rbc; i += 64) dst[i] = *(const uint4*)(stage + s.cent(i / rbc, RB) + (size_t)(i % rbc) * 16);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
int img_write_all(int fd, const void* p, size_t n) {
    const uint8_t* q = (const uint8_t*)p;
    while (n > 0) {
        const ssize_t w = ::write(fd, q, n);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return bb::fail(BBH_ERR_INVALID, "tree image: write failed: %s", std::strerror(errno));
        q += w;
        n -= (size_t)w;
    }
    return BBH_OK;
}

int img_pread_all(int fd, void* p, size_t n, uint64_t off, const char* what) {
    uint8_t* q = (uint8_t*)p;
    while (n > 0) {
        const ssize_t r = ::pread(fd, q, n, (off_t)off);
        if (r < 0 && errno == EINTR) continue;
        if (r < 0) return bb::fail(BBH_ERR_INVALID, "tree image: read failed (%s): %s", what, std::strerror(errno));
        if (r == 0) return bb::fail(BBH_ERR_INVALID, "tree image is truncated (%s)", what);
        q += r;
        n -= (size_t)r;
        off += (uint64_t)r;
    }
    return BBH_OK;
}

// Everything bbh_tree_image_check_fd promises, on the image that starts at byte `base` of `fd`: host code only.
int img_check(int fd, uint64_t base, ImgHeader* out) {
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return bb::fail(BBH_ERR_INVALID, "tree image: the descriptor must be a regular (seekable) file");
    const uint64_t fsize = (uint64_t)st.st_size;
    ImgHeader H;
    if (base > fsize || fsize - base < sizeof(H)) return bb::fail(BBH_ERR_INVALID, "tree image is truncated (header)");
    BB_TRY(img_pread_all(fd, &H, sizeof(H), base, "header"));
    if (std::memcmp(H.magic, IMG_MAGIC, 8) != 0) return bb::fail(BBH_ERR_INVALID, "not a tree image (wrong magic)");
    if (H.endian != IMG_ENDIAN) return bb::fail(BBH_ERR_INVALID, "tree image: byte order mark %08x, expected %08x (little-endian images only)", H.endian, IMG_ENDIAN);
    if (H.version != IMG_VERSION) return bb::fail(BBH_ERR_INVALID, "tree image version %u is not supported (this library reads version %u)", H.version, IMG_VERSION);
    if (H.header_bytes != sizeof(H) || H.group_blocks != IMG_GB || H.ng != NG)
        return bb::fail(BBH_ERR_INVALID, "tree image: header geometry %u / %u / %u, expected %zu / %u / %u", H.header_bytes, H.group_blocks, H.ng, sizeof(H), IMG_GB, NG);
    if (H.F < 8 || H.F % 8 != 0 || H.F > 8192) return bb::fail(BBH_ERR_INVALID, "tree image: n_features %d", H.F);
    if (H.bf < 2 || H.bf > MAX_BF) return bb::fail(BBH_ERR_INVALID, "tree image: branching factor %d", H.bf);
    if (H.crit < 0 || H.crit > BBH_CRIT_NEVER) return bb::fail(BBH_ERR_INVALID, "tree image: merge criterion %d", H.crit);
    if (H.tol_len < 0 || H.tol_len > (1 << 24)) return bb::fail(BBH_ERR_INVALID, "tree image: tolerance table of %d entries", H.tol_len);
    const uint32_t RB = (uint32_t)((H.F / 8 + 15) / 16 * 16), T = H.n_blocks, rows = (uint32_t)H.bf + 1;
    if (H.rb != RB) return bb::fail(BBH_ERR_INVALID, "tree image: row bytes %u, n_features %d needs %u", H.rb, H.F, RB);
    if (T > 0x3FFFFFFFu || H.n8 > 0x3FFFFFFFu || H.n16 > 0x3FFFFFFFu || H.n32 > 0x3FFFFFFFu) return bb::fail(BBH_ERR_INVALID, "tree image: counts beyond 2^30");
    const uint64_t F = (uint64_t)H.F, BB = img_block_bytes(RB);
    const uint64_t want[5] = {(uint64_t)H.tol_len * 8, (uint64_t)T * BB, (uint64_t)H.n8 * F, (uint64_t)H.n16 * F * 2, (uint64_t)H.n32 * F * 4};
    const uint64_t got[5] = {H.tol_bytes, H.node_bytes, H.cf8_bytes, H.cf16_bytes, H.cf32_bytes};
    static const char* nm[5] = {"tolerance", "nodes", "cf8", "cf16", "cf32"};
    uint64_t total = sizeof(H);
    for (int i = 0; i < 5; ++i) {
        if (got[i] != want[i]) return bb::fail(BBH_ERR_INVALID, "tree image: section %s has %llu bytes, the header's counts give %llu", nm[i], (unsigned long long)got[i], (unsigned long long)want[i]);
        total += want[i];
    }
    if (H.image_bytes != total) return bb::fail(BBH_ERR_INVALID, "tree image: %llu bytes recorded, the sections add up to %llu", (unsigned long long)H.image_bytes, (unsigned long long)total);
    if (fsize - base < total) return bb::fail(BBH_ERR_INVALID, "tree image is truncated: %llu bytes of %llu", (unsigned long long)(fsize - base), (unsigned long long)total);
    const uint32_t depth = H.ctr[C_DEPTH];
    if (depth < 1 || depth > (uint32_t)MAXD) return bb::fail(BBH_ERR_INVALID, "tree image: depth %u", depth);
    if (T == 0) {  // a tree that never received anything: the counters of init_empty, no pools
        if (H.n8 != 0 || H.n16 != 0 || H.n32 != 0 || H.ctr[C_IDS] != 0 || H.ctr[C_NODES] != node_blocks(rows) || H.ctr[C_ROOT] != 0 || H.ctr[C_N8] != 1 ||
            H.ctr[C_N16] != 0 || H.ctr[C_N32] != 0 || depth != 1)
            return bb::fail(BBH_ERR_INVALID, "tree image: an image without nodes must be an empty tree");
        if (out) *out = H;
        return BBH_OK;
    }
    if (H.ctr[C_NODES] != T || H.ctr[C_N8] != H.n8 || H.ctr[C_N16] != H.n16 || H.ctr[C_N32] != H.n32 || H.n8 < 1)
        return bb::fail(BBH_ERR_INVALID, "tree image: counters do not match the section counts");
    // pass 1, group by group: headers and links are kept, row records are checked as they come (the node a row belongs to
    // started at or before its block); centroid rows and cardinalities are never read
    std::vector<NodeHdr> hdr;
    std::vector<uint32_t> link;
    std::vector<RowMeta> rmbuf((size_t)IMG_GB * NG);
    try {
        hdr.resize(T);
        link.resize((size_t)T * NG);
    } catch (...) {
        return bb::fail(BBH_ERR_CAPACITY, "tree image: no host memory for the structure of %u blocks", T);
    }
    const uint64_t nodes_at = base + sizeof(H) + want[0];
    uint64_t n_live = 0, n_leaves = 0;
    uint32_t cur = NONE, cur_end = 0, cur_len = 0;
    bool cur_leaf = false;
    for (uint32_t lo = 0; lo < T; lo += IMG_GB) {
        const ImgSlot s = img_slot(lo, 0, T, RB);
        const uint64_t at = nodes_at + s.base;
        BB_TRY(img_pread_all(fd, &hdr[lo], (size_t)s.m * 16, at, "node headers"));
        BB_TRY(img_pread_all(fd, &link[(size_t)lo * NG], (size_t)s.m * 16, at + (size_t)s.m * 16, "node links"));
        BB_TRY(img_pread_all(fd, rmbuf.data(), (size_t)s.m * 128, at + (size_t)s.m * 32, "row records"));
        for (uint32_t ib = lo; ib < lo + s.m; ++ib) {
            const NodeHdr& h = hdr[ib];
            const uint32_t cap = hw_cap(h.leaf);
            if (cap != 0) {
                if (ib < cur_end) return bb::fail(BBH_ERR_INVALID, "tree image: a node starts at block %u inside the node at block %u", ib, cur);
                if (cap > rows) return bb::fail(BBH_ERR_INVALID, "tree image: node %u has capacity %u, branching factor %d allows %u", ib, cap, H.bf, rows);
                if (h.len > cap) return bb::fail(BBH_ERR_INVALID, "tree image: node %u has length %u above its capacity %u", ib, h.len, cap);
                if ((uint64_t)ib + node_blocks(cap) > T) return bb::fail(BBH_ERR_INVALID, "tree image: node %u reaches beyond the last block", ib);
                cur = ib; cur_end = ib + node_blocks(cap); cur_len = h.len; cur_leaf = (h.leaf & HW_LEAF) != 0;
                ++n_live;
                n_leaves += cur_leaf ? 1 : 0;
            }
            if (ib >= cur_end) continue;  // (a block no node owns)
            for (uint32_t j = 0; j < NG; ++j) {
                const uint32_t r = (ib - cur) * NG + j;
                if (r >= cur_len) break;
                const RowMeta& rm = rmbuf[(size_t)(ib - lo) * NG + j];
                const uint32_t tier = rm.slot >> 30, idx = rm.slot & 0x3FFFFFFFu;
                // (a tracking row lives in the uint32 pool and its word must say so: the kernels load it with cf32_load8, which
                // ignores the tier, but store it back with cf_store8, which dispatches on it)
                if (!cur_leaf && tier != 2) return bb::fail(BBH_ERR_INVALID, "tree image: row %u of internal node %u names a cluster-feature slot of tier %u, tracking rows live in tier 2", r, cur, tier);
                const uint32_t lim = tier == 0 ? H.n8 : (tier == 1 ? H.n16 : (tier == 2 ? H.n32 : 0u));
                if (idx >= lim) return bb::fail(BBH_ERR_INVALID, "tree image: row %u of node %u names cluster-feature slot %u of tier %u, which holds %u", r, cur, idx, tier, lim);
                if (cur_leaf) {  // the insertion kernels take a leaf row's slot from its LINK word (k_tree: "link = CF slot word")
                    const uint32_t lw = link[(size_t)ib * NG + j], ltier = lw >> 30, lidx = lw & 0x3FFFFFFFu;
                    const uint32_t llim = ltier == 0 ? H.n8 : (ltier == 1 ? H.n16 : (ltier == 2 ? H.n32 : 0u));
                    if (lidx >= llim) return bb::fail(BBH_ERR_INVALID, "tree image: the link word of row %u of leaf %u names cluster-feature slot %u of tier %u, which holds %u", r, cur, lidx, ltier, llim);
                }
                if (cur_leaf && rm.sub >= H.ctr[C_IDS]) return bb::fail(BBH_ERR_INVALID, "tree image: row %u of leaf %u has id %u of %u", r, cur, rm.sub, H.ctr[C_IDS]);
            }
        }
    }
    auto live = [&](uint32_t b) { return b < T && hw_cap(hdr[b].leaf) != 0; };
    const uint32_t root = H.ctr[C_ROOT], first = H.ctr[C_FIRST_LEAF];
    if (!live(root)) return bb::fail(BBH_ERR_INVALID, "tree image: the root %u starts no live node", root);
    if (first != NONE && !(live(first) && (hdr[first].leaf & HW_LEAF))) return bb::fail(BBH_ERR_INVALID, "tree image: the first leaf %u starts no live leaf", first);
    // pass 2: chain links of every leaf (an internal node's are leftovers of the leaf it was: nothing reads them), then the
    // tree from the root (every node once, depth) and the leaf chain
    for (uint32_t b = 0; b < T; ++b) {
        if (hw_cap(hdr[b].leaf) == 0 || !(hdr[b].leaf & HW_LEAF)) continue;
        for (const uint32_t q : {hdr[b].prev, hdr[b].next})
            if (q != NONE && !(live(q) && (hdr[q].leaf & HW_LEAF))) return bb::fail(BBH_ERR_INVALID, "tree image: chain link %u of leaf %u starts no live leaf", q, b);
    }
    std::vector<uint8_t> seen(T, 0);
    std::vector<uint32_t> level{root}, next_level;
    seen[root] = 1;
    uint64_t reached = 1;
    for (uint32_t d = 1; !level.empty(); ++d) {
        if (d > depth) return bb::fail(BBH_ERR_INVALID, "tree image: the tree is deeper than the %u levels it records", depth);
        next_level.clear();
        for (const uint32_t b : level) {
            if (hdr[b].leaf & HW_LEAF) {  // (the pipelined kernels descend by the depth counter: every leaf sits on the last level)
                if (d != depth) return bb::fail(BBH_ERR_INVALID, "tree image: leaf %u is on level %u of a tree that records %u levels", b, d, depth);
                continue;
            }
            if (hdr[b].len == 0) return bb::fail(BBH_ERR_INVALID, "tree image: internal node %u has no children", b);
            for (uint32_t r = 0; r < hdr[b].len; ++r) {
                const uint32_t c = link[(size_t)b * NG + r];
                if (!live(c)) return bb::fail(BBH_ERR_INVALID, "tree image: row %u of node %u links to block %u, which starts no live node", r, b, c);
                if (seen[c]) return bb::fail(BBH_ERR_INVALID, "tree image: node %u is reached twice", c);
                seen[c] = 1;
                ++reached;
                next_level.push_back(c);
            }
        }
        level.swap(next_level);
    }
    if (reached != n_live) return bb::fail(BBH_ERR_INVALID, "tree image: %llu of %llu nodes hang off the root", (unsigned long long)reached, (unsigned long long)n_live);
    uint64_t walked = 0;
    for (uint32_t b = first; b != NONE; b = hdr[b].next) {
        if (!(hdr[b].leaf & HW_LEAF)) return bb::fail(BBH_ERR_INVALID, "tree image: the leaf chain visits node %u, which is no leaf", b);
        if (seen[b] == 2 || ++walked > n_leaves) return bb::fail(BBH_ERR_INVALID, "tree image: the leaf chain loops at node %u", b);
        seen[b] = 2;
    }
    if (walked != n_leaves) return bb::fail(BBH_ERR_INVALID, "tree image: the leaf chain visits %llu of %llu leaves", (unsigned long long)walked, (unsigned long long)n_leaves);
    if (out) *out = H;
    return BBH_OK;
}

double img_ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int img_save(bbh_tree* t, int fd, uint64_t stage_bytes, uint64_t* written) {
    const TreeDev& h = t->h;
    const uint32_t RB = (uint32_t)h.RB, rows = (uint32_t)h.bf + 1;
    const uint64_t BB = img_block_bytes(RB), F = (uint64_t)h.F;
    const bool empty = t->lazy_pools || h.node_hdr == nullptr;
    const uint32_t used = empty ? 0u : h.ctr[C_NODES];
    if (!empty && (used > h.cap_nodes || h.ctr[C_N8] > h.cap8 || h.ctr[C_N16] > h.cap16 || h.ctr[C_N32] > h.cap32 || h.ctr[C_ROOT] >= used))
        return bb::fail(BBH_ERR_STATE, "the tree's counters exceed its pools: it cannot be saved");
    bb::DevScope tmp(nullptr);  // device and pinned buffers of the call (the null stream and blocking copies throughout)
    uint32_t *d_sz = nullptr, *d_id = nullptr;
    void* d_tmp = nullptr;
    uint8_t *d_stage = nullptr, *pin = nullptr;
    ImgHeader H;
    std::memset(&H, 0, sizeof(H));
    std::memcpy(H.magic, IMG_MAGIC, 8);
    H.version = IMG_VERSION; H.endian = IMG_ENDIAN; H.header_bytes = sizeof(H); H.group_blocks = IMG_GB;
    H.bf = h.bf; H.F = h.F; H.crit = h.crit; H.tol_len = t->d_tol ? h.tol_len : 0;
    H.ng = NG; H.rb = RB;
    H.thr = h.thr; H.tolerance = h.tolerance;
    for (int i = 0; i < C_COUNT; ++i) H.ctr[i] = h.ctr[i];
    for (int i = 0; i < 8; ++i) H.stats[i] = h.stats[i];
    uint32_t T = 0;
    if (!empty) {
        BB_HIP(tmp.get(&d_sz, ((size_t)used + 1) * 4));
        BB_HIP(tmp.get(&d_id, ((size_t)used + 1) * 4));
        BB_HIP(hipMemset(d_sz + used, 0, 4));
        bb::ProfScope ps("tree_image/save", nullptr);
        hipLaunchKernelGGL(k_img_size, dim3((used + 255) / 256), dim3(256), 0, 0, (const NodeHdr*)h.node_hdr, used, rows, h.ctr[C_ROOT], d_sz);
        BB_HIP(hipGetLastError());
        size_t tmp_bytes = 0;
        BB_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, d_sz, d_id, 0u, (size_t)used + 1, rocprim::plus<uint32_t>(), (hipStream_t)0));
        BB_HIP(tmp.get(&d_tmp, tmp_bytes + 16));
        BB_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, d_sz, d_id, 0u, (size_t)used + 1, rocprim::plus<uint32_t>(), (hipStream_t)0));
        uint32_t new_root = 0, new_first = NONE;
        BB_HIP(hipMemcpy(&T, d_id + used, 4, hipMemcpyDeviceToHost));
        BB_HIP(hipMemcpy(&new_root, d_id + h.ctr[C_ROOT], 4, hipMemcpyDeviceToHost));
        if (h.ctr[C_FIRST_LEAF] != NONE && h.ctr[C_FIRST_LEAF] < used) BB_HIP(hipMemcpy(&new_first, d_id + h.ctr[C_FIRST_LEAF], 4, hipMemcpyDeviceToHost));
        if (T == 0 || T > 0x3FFFFFFFu) return bb::fail(BBH_ERR_STATE, "the tree holds no live node: it cannot be saved");
        H.n_blocks = T; H.n8 = h.ctr[C_N8]; H.n16 = h.ctr[C_N16]; H.n32 = h.ctr[C_N32];
        H.ctr[C_NODES] = T; H.ctr[C_ROOT] = new_root; H.ctr[C_FIRST_LEAF] = new_first;
        ps.units((long long)sizeof(H));
    }
    H.tol_bytes = (uint64_t)H.tol_len * 8; H.node_bytes = (uint64_t)T * BB;
    H.cf8_bytes = (uint64_t)H.n8 * F; H.cf16_bytes = (uint64_t)H.n16 * F * 2; H.cf32_bytes = (uint64_t)H.n32 * F * 4;
    H.image_bytes = sizeof(H) + H.tol_bytes + H.node_bytes + H.cf8_bytes + H.cf16_bytes + H.cf32_bytes;
    BB_TRY(img_write_all(fd, &H, sizeof(H)));
    if (H.tol_len > 0) {
        std::vector<double> tab((size_t)H.tol_len);
        BB_HIP(hipMemcpy(tab.data(), t->d_tol, H.tol_bytes, hipMemcpyDeviceToHost));
        BB_TRY(img_write_all(fd, tab.data(), H.tol_bytes));
    }
    if (!empty) {
        const uint32_t n_groups = (T + IMG_GB - 1) / IMG_GB;
        const uint64_t stage = stage_bytes ? stage_bytes : IMG_DEFAULT_STAGE;
        const uint32_t per = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(stage / (IMG_GB * BB), 1), n_groups);
        const size_t buf_bytes = (size_t)per * IMG_GB * BB;
        BB_HIP(tmp.get(&d_stage, buf_bytes));
        BB_HIP(tmp.pinned(&pin, buf_bytes));
        note_peak(t, buf_bytes + ((size_t)used + 1) * 8);
        for (uint32_t g = 0; g < n_groups; g += per) {
            const uint32_t lo = g * IMG_GB, hi = (uint32_t)std::min<uint64_t>(T, ((uint64_t)g + per) * IMG_GB);
            const size_t bytes = (size_t)(hi - lo) * BB;
            {
                bb::ProfScope ps("tree_image/save", nullptr);
                ps.units((long long)bytes);
                BB_HIP(hipMemsetAsync(d_stage, 0, bytes, nullptr));
                const uint32_t grid = std::min<uint32_t>(std::max<uint32_t>((hi - lo) / 4, 1u), 1u << 14);
                hipLaunchKernelGGL(k_img_pack, dim3(grid), dim3(256), 0, 0, h, used, rows, (const uint32_t*)d_sz, (const uint32_t*)d_id, T, lo, hi, d_stage);
                BB_HIP(hipGetLastError());
            }
            BB_HIP(hipMemcpy(pin, d_stage, bytes, hipMemcpyDeviceToHost));
            BB_TRY(img_write_all(fd, pin, bytes));
        }
        // the cluster-feature pools go out as they lie: their used prefixes, through the same pinned buffer
        const uint8_t* pools[3] = {(const uint8_t*)h.cf8, (const uint8_t*)h.cf16, (const uint8_t*)h.cf32};
        const uint64_t sizes[3] = {H.cf8_bytes, H.cf16_bytes, H.cf32_bytes};
        bb::ProfScope ps("tree_image/save", nullptr);
        ps.units((long long)(H.tol_bytes + sizes[0] + sizes[1] + sizes[2]));
        for (int p = 0; p < 3; ++p)
            for (uint64_t off = 0; off < sizes[p]; off += buf_bytes) {
                const size_t bytes = (size_t)std::min<uint64_t>(buf_bytes, sizes[p] - off);
                BB_HIP(hipMemcpy(pin, pools[p] + off, bytes, hipMemcpyDeviceToHost));
                BB_TRY(img_write_all(fd, pin, bytes));
            }
    }
    if (written) *written = H.image_bytes;
    return BBH_OK;
}

int img_load(bbh_tree* t, int fd, uint64_t base, const ImgHeader& H, uint64_t stage_bytes) {
    TreeDev& h = t->h;
    const uint32_t T = H.n_blocks, RB = (uint32_t)h.RB, rows = (uint32_t)h.bf + 1;
    const uint64_t BB = img_block_bytes(RB), F = (uint64_t)h.F;
    uint64_t at = base + sizeof(H);
    if (H.tol_len > 0) {
        std::vector<double> tab((size_t)H.tol_len);
        BB_TRY(img_pread_all(fd, tab.data(), H.tol_bytes, at, "tolerance table"));
        BB_TRY(set_tol(t, tab.data(), H.tol_len));
    }
    at += H.tol_bytes;
    if (T == 0) return BBH_OK;
    bb::DevScope tmp(nullptr);  // (as in img_save)
    uint8_t *d_stage = nullptr, *pin = nullptr;
    const uint32_t n_groups = (T + IMG_GB - 1) / IMG_GB;
    const uint64_t stage = stage_bytes ? stage_bytes : IMG_DEFAULT_STAGE;
    const uint32_t per = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(stage / (IMG_GB * BB), 1), n_groups);
    const size_t buf_bytes = (size_t)per * IMG_GB * BB;
    BB_HIP(tmp.get(&d_stage, buf_bytes));
    BB_HIP(tmp.pinned(&pin, buf_bytes));
    // the cluster-feature pools first (what they hold and the room a first insertion needs, as grow_cf's floor), then the
    // node pools as gc_nodes sizes its new ones: everything live plus a quarter, within what the device has free
    const uint32_t depth = H.ctr[C_DEPTH];
    const uint32_t spare = tiny_pools() ? 8u : 2 * depth + 64;
    const uint32_t caps[3] = {clamp30((uint64_t)H.n8 + spare), clamp30((uint64_t)H.n16 + spare), clamp30((uint64_t)H.n32 + spare)};
    BB_TRY(grow_pool((void**)&h.cf8, 1, 0, (size_t)caps[0] * F));
    h.cap8 = caps[0];
    BB_TRY(grow_pool((void**)&h.cf16, 2, 0, (size_t)caps[1] * F));
    h.cap16 = caps[1];
    BB_TRY(grow_pool((void**)&h.cf32, 4, 0, (size_t)caps[2] * F));
    h.cap32 = caps[2];
    const uint64_t floor_b = (uint64_t)T + (2 * (uint64_t)depth + 8) * node_blocks(rows);
    uint64_t want = std::max<uint64_t>((uint64_t)T + (tiny_pools() ? 0 : (uint64_t)T / 4), floor_b);
    size_t free_b = 0;
    if (bb::dev_free_bytes((size_t)((double)want * (double)BB / 0.92) + 1, &free_b) == hipSuccess) {
        const uint64_t room = (uint64_t)((double)free_b * 0.92) / BB;
        if (want > room) {
            if (room < floor_b)
                return bb::fail(BBH_ERR_CAPACITY, "out of device memory: the image's node pools hold %.2f GB and %.2f GB are free", (double)T * (double)BB / 1e9, (double)free_b / 1e9);
            want = room;
        }
    } else {
        (void)hipGetLastError();
    }
    if (want > 0x3FFFFFFFull) want = 0x3FFFFFFFull;
    if (want < floor_b) return bb::fail(BBH_ERR_CAPACITY, "node pool limit of 2^30 blocks reached");
    BB_TRY(realloc_node_pools(t, 0, (size_t)want));
    note_peak(t, buf_bytes);
    for (uint32_t g = 0; g < n_groups; g += per) {
        const uint32_t lo = g * IMG_GB, hi = (uint32_t)std::min<uint64_t>(T, ((uint64_t)g + per) * IMG_GB);
        const size_t bytes = (size_t)(hi - lo) * BB;
        BB_TRY(img_pread_all(fd, pin, bytes, at, "nodes"));
        BB_HIP(hipMemcpy(d_stage, pin, bytes, hipMemcpyHostToDevice));
        bb::ProfScope ps("tree_image/load", nullptr);
        ps.units((long long)(bytes + (g == 0 ? sizeof(H) + H.tol_bytes : 0)));
        const uint32_t grid = std::min<uint32_t>(std::max<uint32_t>((hi - lo) / 4, 1u), 1u << 14);
        hipLaunchKernelGGL(k_img_unpack, dim3(grid), dim3(256), 0, 0, h, T, lo, hi, (const uint8_t*)d_stage);
        BB_HIP(hipGetLastError());
        at += bytes;
    }
    {
        uint8_t* pools[3] = {(uint8_t*)h.cf8, (uint8_t*)h.cf16, (uint8_t*)h.cf32};
        const uint64_t sizes[3] = {H.cf8_bytes, H.cf16_bytes, H.cf32_bytes};
        bb::ProfScope ps("tree_image/load", nullptr);
        ps.units((long long)(sizes[0] + sizes[1] + sizes[2]));
        for (int p = 0; p < 3; ++p)
            for (uint64_t off = 0; off < sizes[p]; off += buf_bytes) {
                const size_t bytes = (size_t)std::min<uint64_t>(buf_bytes, sizes[p] - off);
                BB_TRY(img_pread_all(fd, pin, bytes, at, "cluster features"));
                BB_HIP(hipMemcpy(pools[p] + off, pin, bytes, hipMemcpyHostToDevice));
                at += bytes;
            }
    }
    BB_HIP(hipDeviceSynchronize());
    for (int i = 0; i < C_COUNT; ++i) h.ctr[i] = H.ctr[i];
    for (int i = 0; i < 8; ++i) h.stats[i] = H.stats[i];
    t->lazy_pools = false;
    t->chain_valid = false;
    return BBH_OK;
}

}  // namespace

extern "C" int bbh_tree_image_check_fd(int fd, uint64_t* image_bytes) {
    const off_t base = lseek(fd, 0, SEEK_CUR);
    if (base < 0) return bb::fail(BBH_ERR_INVALID, "tree image: the descriptor must be a regular (seekable) file");
    ImgHeader H;
    BB_TRY(img_check(fd, (uint64_t)base, &H));
    if (image_bytes) *image_bytes = H.image_bytes;
    return BBH_OK;
}

extern "C" int bbh_tree_save_fd(bbh_tree* t, int fd, uint64_t stage_bytes, uint64_t* written) {
    if (!t) return bb::fail(BBH_ERR_INVALID, "null tree");
    if (stage_bytes != 0 && stage_bytes < BBH_TREE_IMAGE_MIN_STAGE(t->h.F))
        return bb::fail(BBH_ERR_INVALID, "stage_bytes %llu is below one group of the image (%llu bytes for %d features)", (unsigned long long)stage_bytes,
                        (unsigned long long)BBH_TREE_IMAGE_MIN_STAGE(t->h.F), t->h.F);
    BB_HIP(hipSetDevice(t->device));
    BB_HIP(hipDeviceSynchronize());
    return img_save(t, fd, stage_bytes, written);
}

extern "C" int bbh_tree_load_fd(bbh_tree** out, int fd, int32_t device, uint64_t stage_bytes) {
    if (out == nullptr) return bb::fail(BBH_ERR_INVALID, "null output handle");
    *out = nullptr;
    const off_t base = lseek(fd, 0, SEEK_CUR);
    if (base < 0) return bb::fail(BBH_ERR_INVALID, "tree image: the descriptor must be a regular (seekable) file");
    ImgHeader H;
    BB_TRY(img_check(fd, (uint64_t)base, &H));  // (before the device is touched: a bad image never reaches a kernel)
    if (stage_bytes != 0 && stage_bytes < BBH_TREE_IMAGE_MIN_STAGE(H.F))
        return bb::fail(BBH_ERR_INVALID, "stage_bytes %llu is below one group of the image (%llu bytes for %d features)", (unsigned long long)stage_bytes,
                        (unsigned long long)BBH_TREE_IMAGE_MIN_STAGE(H.F), H.F);
    BB_TRY(bb::ensure_device());
    BB_HIP(hipSetDevice(device));
    bbh_tree* t = new bbh_tree();
    t->device = device;
    t->h.thr = H.thr;
    t->h.crit = H.crit;
    t->h.tolerance = H.tolerance;
    int rc = configure(t, H.bf, H.F);
    if (rc == BBH_OK) {
        hipError_t e = bb::dev_alloc(&t->d, sizeof(TreeDev));
        if (e != hipSuccess) rc = bb::fail(BBH_ERR_HIP, "hipMalloc: %s", hipGetErrorString(e));
    }
    if (rc == BBH_OK) rc = init_empty(t);
    if (rc == BBH_OK) rc = img_load(t, fd, (uint64_t)base, H, stage_bytes);
    if (rc == BBH_OK && lseek(fd, (off_t)((uint64_t)base + H.image_bytes), SEEK_SET) < 0) rc = bb::fail(BBH_ERR_INVALID, "tree image: seek failed");
    if (rc != BBH_OK) {
        bbh_tree_destroy(t);
        return rc;
    }
    *out = t;
    return BBH_OK;
}
