// bb_components.hip -- the connected components of a packed table at a Jaccard distance, for gfx950 (MI355X, CDNA4): the
// consumer of bb_radius.hip's graph that never stores an edge.  DESIGN.md section 5h.
//
//   bbh_jt_components    root (smallest row of the component), label (rank of the root) and the number of components
//     k_radius_table     imin[u], the smallest passing intersection of every union (bb_radius_common.h)
//     k_cc_init          parent[v] = v
//     k_cc_pairs         AND + popcount, lane per row, for the usual widths (k_radius_bcnt's counting loop) over the upper
//                        triangle m > q; the pass test is i >= imin[u] out of LDS; a hit unites the two rows
//     k_cc_pairs_generic every other width and alignment: one wave per row, the float64 division itself, lane 0 unites
//     k_cc_flatten       root[v] = find(v), in a launch of its own
//     k_cc_scan          one workgroup: rank[v] = roots below v, and their number
//     k_cc_label         label[v] = rank[root[v]]
//
// Rows a and b are linked iff bbh_jt_radius reports the pair: jaccard_dist(i, u) <= radius in float64.  The components are
// the transitive closure.  The union-find is lock-free and never waits: a thread only follows parent[] downwards and
// exchanges a root's own entry by compare-and-swap, "larger under smaller".  Two invariants carry the design:
//
//   I1  Every value ever stored in parent[v] is <= v and is a row of v's component.
//       (k_cc_init stores v.  A CAS stores lo < hi into parent[hi], lo and hi being rows reached from a linked pair by
//       values stored earlier.  Path halving stores parent[parent[v]], both read from stored values, with atomicMin: <= v.)
//   I2  A root stops being a root only through a successful CAS (parent[hi]: hi -> lo < hi), and never becomes one again:
//       halving touches parent[v] only after a value != v was read from it, and stores values < v.
//
// Nothing rests on a load being fresh (the L2s of the XCDs are not coherent with each other, a CU's L1 is never refreshed);
// only on the CAS being atomic at agent scope.  A stale load of parent[v] returns an earlier value, which by I1 is a row
// <= v that v has been tied to, and ties are never undone (halving replaces a parent by that parent's parent): so whatever
// find(v) returns is in v's tree for good.  If find(a) == find(b) the two are in one tree and there is nothing to do.
// Otherwise the CAS on the larger candidate succeeds exactly when that row still is a root (I2), which ties the trees; a CAS
// that fails returns the entry's current value, smaller than the candidate, and the loop goes on from there: every turn
// lowers an index, no turn depends on another thread's progress.  When k_cc_pairs is over every linked pair shares a tree,
// by I1 a tree never leaves a component, and a root is the smallest row of its tree because parents are smaller than
// children.  k_cc_flatten runs after the kernel boundary, reads the final parent[] and writes nothing find() reads.
// The result is a function of the rows and the radius alone: not of the kernel, the grid or the order of the workgroups.
// No fences, no flags, no hand-over between workgroups, no inline assembly.
#include "bb_common.h"
#include "bb_radius_common.h"  // jaccard_dist, k_radius_table, radius_ranges

using namespace bbd;

namespace {

// (relaxed, agent scope: served by L2, not by the CU's L1; correctness does not need it, fewer failed CAS do)
__device__ __forceinline__ int cc_load(const int* parent, int v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above v as far as this thread can see, halving the path on the way; v strictly decreases
template <bool HALVE>
__device__ __forceinline__ int cc_find(int* parent, int v) {
    int p = cc_load(parent, v);
    while (p != v) {
        const int g = cc_load(parent, p);
        if (HALVE && g != p) atomicMin(&parent[v], g);
        v = p;
        p = g;
    }
    return v;
}

// ties the trees of a and b; returns the root they share as far as this thread can see.  max(ra, rb) strictly decreases.
__device__ __forceinline__ int cc_unite(int* parent, int a, int b) {
    int ra = cc_find<true>(parent, a), rb = cc_find<true>(parent, b);
    while (ra != rb) {
        const int hi = max(ra, rb), lo = min(ra, rb);
        const int old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return lo;
        ra = cc_find<true>(parent, old);  // hi was no root any more: old < hi is above it
        rb = lo;
    }
    return ra;
}

// The ranges of the pair kernels: bbh_jt_radius's rule, but the device filled 64 times over instead of 4.  Half of a
// triangle's grid returns at once and the rest is uneven (a block near the diagonal has a fraction of a range), so the
// blocks must outnumber the device's slots for the dispatcher to even them out; measured in DESIGN.md 5h.
constexpr int CC_FILL = 64;

__global__ __launch_bounds__(256) void k_cc_init(int n, int* __restrict__ parent) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) parent[v] = (int)v;
}

// ---------------------------------------------------------------------------------------------------------------
// AND + popcount over the upper triangle.  Every lane owns row q in registers and meets the rows m > q of its range;
// table rows are wave-uniform (scalar loads).  Grid: x = tiles of 256 rows, y = table ranges.  The union is inline behind
// a filter: the lane keeps the last root it saw for q and skips where parent[m] or its parent is that root.
// ---------------------------------------------------------------------------------------------------------------
template <int W32>
__global__ __launch_bounds__(256) void k_cc_pairs(const uint32_t* __restrict__ c, int n, int per_range,
                                                  const uint32_t* __restrict__ ccard,
                                                  const uint16_t* __restrict__ tab, int* parent) {
    __shared__ uint16_t imin[W32 * 32 + 2];
    const int tid = (int)threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * 256;
    const int m1 = (int)min((int64_t)n, ((int64_t)blockIdx.y + 1) * per_range);
    if ((int64_t)m1 - 1 <= q0) return;  // the whole range lies at or below the tile
    for (int u = tid; u <= W32 * 32; u += 256) imin[u] = tab[u];
    const int64_t qi = q0 + tid;
    const bool ok = qi < n;
    const uint32_t* src = c + (size_t)(ok ? qi : 0) * W32;
    uint32_t x[W32];
    uint32_t qc = 0;
#pragma unroll
    for (int w = 0; w < W32; ++w) {
        x[w] = ok ? src[w] : 0u;
        qc += __popc(x[w]);
    }
    __syncthreads();
    // the wave's first row with a partner: its lowest lane's q + 1
    const int64_t first = q0 + (tid & ~63) + 1;
    const int m0 = (int)min((int64_t)m1, max((int64_t)blockIdx.y * per_range, first));
    const int self = ok ? (int)qi : 0x7fffffff;
    int known = self;  // the last root seen above q
    // (one row at a time: interleaving two rows of the counting loop doubles its registers and halves the waves per SIMD)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int m = m0; m < m1; ++m) {
        const uint32_t* cr = c + (size_t)m * W32;  // wave-uniform address
        uint32_t inter = 0;
#pragma unroll
        for (int w = 0; w < W32; ++w) inter += __popc(x[w] & cr[w]);
        const uint32_t un = qc + ccard[m] - inter;
        if (inter >= (uint32_t)imin[un] && m > self) {
            const int pm = cc_load(parent, m);
            if (pm != known && cc_load(parent, pm) != known) known = cc_unite(parent, self, m);
        }
    }
}

// any width, any alignment: one wave per row, lanes stride over the bytes of every later row of the range; every lane
// holds the pair's counts after the wave sums, lane 0 unites
__global__ __launch_bounds__(256) void k_cc_pairs_generic(const uint8_t* __restrict__ c, int n, int per_range,
                                                          int64_t nbytes, const uint32_t* __restrict__ ccard,
                                                          double radius, int* parent) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= n) return;
    const int m1 = (int)min((int64_t)n, ((int64_t)blockIdx.y + 1) * per_range);
    const int m0 = (int)max((int64_t)blockIdx.y * per_range, qi + 1);
    if (m0 >= m1) return;
    const uint8_t* qr = c + (size_t)qi * nbytes;
    const uint32_t qc = ccard[qi];
    int known = (int)qi;
    for (int m = m0; m < m1; ++m) {
        const uint8_t* cr = c + (size_t)m * nbytes;
        uint32_t inter = 0;
        for (int64_t j = lane; j < nbytes; j += 64) inter += __popc((uint32_t)(qr[j] & cr[j]));
        inter = wave_sum_u32(inter);
        const uint32_t un = qc + ccard[m] - inter;
        if (!(jaccard_dist(inter, un) <= radius)) continue;
        if (lane == 0) {
            const int pm = cc_load(parent, m);
            if (pm != known && cc_load(parent, pm) != known) known = cc_unite(parent, (int)qi, m);
        }
    }
}

// after the pair kernel has ended: every entry is final, nothing is stored that find() reads
__global__ __launch_bounds__(256) void k_cc_flatten(int n, int* parent, int32_t* __restrict__ root) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) root[v] = cc_find<false>(parent, (int)v);
}

// One workgroup (k_radius_scan with 32-bit entries): rank[v] = the number of roots below v, 1024 rows a turn with a running
// carry, and the number of roots.  A few hundred turns of a microsecond for a million rows.
__global__ __launch_bounds__(1024) void k_cc_scan(int n, const int32_t* __restrict__ root, int* __restrict__ rank,
                                                  int64_t* __restrict__ count) {
    __shared__ int wsum[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const int flag = (i < n && root[i] == (int)i) ? 1 : 0;
        int v = flag;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int t = wsum[w];
            before += w < wave ? t : 0;
            all += t;
        }
        if (rank != nullptr && i < n) rank[i] = carry + before + v - flag;
        carry += all;
        __syncthreads();
    }
    if (tid == 0 && count != nullptr) *count = carry;
}

__global__ __launch_bounds__(256) void k_cc_label(int n, const int32_t* __restrict__ root, const int* __restrict__ rank,
                                                  int32_t* __restrict__ label) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) label[v] = rank[root[v]];
}

}  // namespace

extern "C" int bbh_jt_components(const uint8_t* rows, int64_t n, int64_t nbytes, double radius, int32_t* out_root,
                                 int32_t* out_label, int64_t* out_count, void* stream) {
    BB_TRY(bb::ensure_device());
    if (n < 0 || n > 0x7fffffffLL || nbytes <= 0)
        return bb::fail(BBH_ERR_INVALID, "components: need 0 <= n < 2^31 and nbytes > 0");
    if (radius != radius) return bb::fail(BBH_ERR_INVALID, "components: the radius is NaN");
    if (out_root == nullptr && out_label == nullptr && out_count == nullptr)
        return bb::fail(BBH_ERR_INVALID, "components: need a root, a label or a count output");
    if (n > 0 && rows == nullptr) return bb::fail(BBH_ERR_INVALID, "components: no rows");
    hipStream_t s = (hipStream_t)stream;
    bb::DevIn c;
    bb::DevOut orr, ol, oc;
    BB_TRY(oc.init(out_count, 8));
    bb::DevScope tmp(s);
    if (n == 0) {
        if (oc.dev) BB_HIP(hipMemsetAsync(oc.dev, 0, 8, s));
        BB_TRY(oc.finish(s));
        return tmp.sync();
    }
    BB_TRY(orr.init(out_root, (size_t)n * 4));
    BB_TRY(ol.init(out_label, (size_t)n * 4));
    BB_TRY(c.init(rows, (size_t)(n * nbytes), s));
    const uint8_t* cd = (const uint8_t*)c.dev;
    const bool fast = (uintptr_t)cd % 4 == 0 && radius_fast_width(nbytes);

    uint32_t* ccard = nullptr;
    BB_HIP(tmp.get(&ccard, (size_t)n * 4));
    BB_TRY(bbh_popcount_rows(cd, n, nbytes, nbytes, ccard, s));
    {
        bb::ProfScope ps("jt_components", s);
        ps.units(n);
        int64_t qblocks = 0;
        int per = 0, nsplit = 0;
        radius_ranges(n, n, fast, CC_FILL, &qblocks, &per, &nsplit);
        int* parent = nullptr;  // the forest; after k_cc_flatten the ranks of the roots
        int32_t* root = (int32_t*)orr.dev;
        uint16_t* tab = nullptr;
        BB_HIP(tmp.get(&parent, (size_t)n * 4));
        if (root == nullptr) BB_HIP(tmp.get(&root, (size_t)n * 4));
        const dim3 flat((unsigned)((n + 255) / 256));
        // (u - i) / u lies in [0, 1] for every pair: a radius >= 1 links all rows (every parent is row 0), a radius < 0 none
        const bool all = radius >= 1.0, none = radius < 0.0;
        if (all) {
            BB_HIP(hipMemsetAsync(parent, 0, (size_t)n * 4, s));
        } else {
            hipLaunchKernelGGL(k_cc_init, flat, dim3(256), 0, s, (int)n, parent);
            BB_HIP(hipGetLastError());
        }
        if (fast && !all && !none) {
            const int nbits = (int)nbytes * 8;
            BB_HIP(tmp.get(&tab, (size_t)(nbits + 1) * 2));
            hipLaunchKernelGGL(k_radius_table, dim3((unsigned)(nbits / 256 + 1)), dim3(256), 0, s, radius, nbits, tab);
            BB_HIP(hipGetLastError());
        }
        const dim3 grid((unsigned)qblocks, (unsigned)nsplit);
#define BB_LAUNCH_CC(W) \
    hipLaunchKernelGGL((k_cc_pairs<W>), grid, dim3(256), 0, s, (const uint32_t*)cd, (int)n, per, ccard, tab, parent)
        if (all || none) (void)grid;  // nothing to meet
        else if (!fast)
            hipLaunchKernelGGL(k_cc_pairs_generic, grid, dim3(256), 0, s, cd, (int)n, per, nbytes, ccard, radius, parent);
        else if (nbytes == 8) BB_LAUNCH_CC(2);
        else if (nbytes == 16) BB_LAUNCH_CC(4);
        else if (nbytes == 32) BB_LAUNCH_CC(8);
        else if (nbytes == 64) BB_LAUNCH_CC(16);
        else if (nbytes == 128) BB_LAUNCH_CC(32);
        else BB_LAUNCH_CC(64);
#undef BB_LAUNCH_CC
        BB_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cc_flatten, flat, dim3(256), 0, s, (int)n, parent, root);
        BB_HIP(hipGetLastError());
        if (ol.dev != nullptr || oc.dev != nullptr) {
            int* rank = ol.dev != nullptr ? parent : nullptr;  // (the forest is done with)
            hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(1024), 0, s, (int)n, root, rank, (int64_t*)oc.dev);
            BB_HIP(hipGetLastError());
        }
        if (ol.dev != nullptr) {
            hipLaunchKernelGGL(k_cc_label, flat, dim3(256), 0, s, (int)n, root, parent, (int32_t*)ol.dev);
            BB_HIP(hipGetLastError());
        }
    }
    BB_TRY(orr.finish(s));
    BB_TRY(ol.finish(s));
    BB_TRY(oc.finish(s));
    return tmp.sync();
}
