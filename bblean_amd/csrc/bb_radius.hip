// bb_radius.hip -- every row of a table within a Jaccard distance of every query, for gfx950 (MI355X, CDNA4): the
// threshold twin of bb_topk.hip, with an output whose size is not known before the call.  DESIGN.md section 5f.
//
//   bbh_jt_radius        CSR (offsets, idx, inter, union) of the pairs with (u - i) / u <= radius
//     k_radius_table     imin[u], the smallest passing intersection of every union: one thread per u, once per call
//     k_radius_bcnt      AND + popcount, lane per query, for the usual widths (k_assign_bcnt's inner loop); the pass test
//                        is i >= imin[u] out of LDS, no division.  FILL = false counts, FILL = true writes
//     k_radius_generic   every other width and alignment: one wave per query, the float64 division itself
//     k_radius_sum       per query: the counts of the table ranges -> their exclusive prefix (in place) and the sum
//     k_radius_scan      the sums -> the int64 offsets and the total
//
// A pair is a hit iff jaccard_dist(i, u) <= radius in float64, where jaccard_dist is bbh_jt_dist_matrix's single division
// and 0.0 where u == 0.  Rounding is monotone, so for a fixed u the quotient does not increase with i and the hits are
// exactly i >= imin[u]; imin[u] = u + 1 where no i passes.
//
// Two passes instead of atomics: the count pass leaves part[range][q]; after the two scan steps a lane of the fill pass
// knows where its hits start, walks its range again and writes them in ascending row index.  The output therefore does
// not depend on the order in which workgroups run, nor (ranges ascend too) on how the table was split.
#include "bb_common.h"
#include "bb_radius_common.h"  // jaccard_dist, k_radius_table, radius_ranges

using namespace bbd;

namespace {

// ---------------------------------------------------------------------------------------------------------------
// AND + popcount.  Every lane owns one query row in registers; table rows are wave-uniform (scalar loads).  Grid:
// x = query tiles of 256, y = table ranges.  The workgroup stages imin in LDS (at most 2049 entries of 16 bits).
// FILL = false: part[range][q] = hits of the lane in its range.  FILL = true: part holds the exclusive prefix over the
// ranges; the lane writes from offsets[q] + part[range][q] upwards and stops short of offsets[q + 1] or of the next
// range's start by construction: it meets the same hits as the count pass did.
// ---------------------------------------------------------------------------------------------------------------
template <int W32, bool FILL>
__global__ __launch_bounds__(256) void k_radius_bcnt(const uint8_t* __restrict__ q, int64_t nq, int64_t q_stride,
                                                     const uint32_t* __restrict__ c, int nc, int per_range,
                                                     const uint32_t* __restrict__ ccard,
                                                     const uint16_t* __restrict__ tab,
                                                     const int32_t* __restrict__ exclude, int* __restrict__ part,
                                                     const int64_t* __restrict__ offsets, int32_t* __restrict__ out_idx,
                                                     uint32_t* __restrict__ out_inter, uint32_t* __restrict__ out_union) {
    __shared__ uint16_t imin[W32 * 32 + 2];
    const int tid = (int)threadIdx.x;
    for (int u = tid; u <= W32 * 32; u += 256) imin[u] = tab[u];
    const int64_t qi = (int64_t)blockIdx.x * 256 + tid;
    const bool ok = qi < nq;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(q + (ok ? qi : 0) * q_stride);
    uint32_t x[W32];
    uint32_t qc = 0;
#pragma unroll
    for (int w = 0; w < W32; ++w) {
        x[w] = ok ? src[w] : 0u;
        qc += __popc(x[w]);
    }
    const int ex = (ok && exclude != nullptr) ? exclude[qi] : -1;
    const int64_t slot = (int64_t)blockIdx.y * nq + qi;
    int64_t pos = 0, end = 0;
    if (FILL) {
        // the lane's hits: the next range's start (or the query's end) minus its own
        if (ok) {
            pos = offsets[qi] + part[slot];
            end = blockIdx.y + 1 < gridDim.y ? offsets[qi] + part[slot + nq] : offsets[qi + 1];
        }
        __syncthreads();
        if (!__any(end > pos)) return;  // nothing to write in this wave's part of the range
    } else {
        __syncthreads();
    }
    const int m0 = (int)blockIdx.y * per_range;
    const int m1 = (int)min((int64_t)nc, (int64_t)m0 + per_range);
    int cnt = 0;
    // (one row at a time: interleaving two rows of the counting loop doubles its registers and halves the waves per SIMD)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int m = m0; m < m1; ++m) {
        const uint32_t* cr = c + (size_t)m * W32;  // wave-uniform address
        uint32_t inter = 0;
#pragma unroll
        for (int w = 0; w < W32; ++w) inter += __popc(x[w] & cr[w]);
        const uint32_t un = qc + ccard[m] - inter;
        const bool hit = inter >= (uint32_t)imin[un] && m != ex;
        if (FILL) {
            if (hit && pos < end) {  // (pos < end always where the lane has a query: it meets the count pass's hits)
                out_idx[pos] = m;
                if (out_inter) out_inter[pos] = inter;
                if (out_union) out_union[pos] = un;
                ++pos;
            }
        } else {
            cnt += hit ? 1 : 0;
        }
    }
    if (!FILL && ok) part[slot] = cnt;
}

// any width, any alignment: one wave per query, lanes stride over the bytes of every row of the range; every lane holds
// the pair's counts after the wave sums, lane 0 writes
template <bool FILL>
__global__ __launch_bounds__(256) void k_radius_generic(const uint8_t* __restrict__ q, int64_t nq, int64_t q_stride,
                                                        const uint8_t* __restrict__ c, int nc, int per_range,
                                                        int64_t nbytes, const uint32_t* __restrict__ ccard,
                                                        double radius, const int32_t* __restrict__ exclude,
                                                        int* __restrict__ part, const int64_t* __restrict__ offsets,
                                                        int32_t* __restrict__ out_idx, uint32_t* __restrict__ out_inter,
                                                        uint32_t* __restrict__ out_union) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const uint8_t* qr = q + qi * q_stride;
    uint32_t qc = 0;
    for (int64_t j = lane; j < nbytes; j += 64) qc += __popc((uint32_t)qr[j]);
    qc = wave_sum_u32(qc);
    const int ex = exclude != nullptr ? exclude[qi] : -1;
    const int64_t slot = (int64_t)blockIdx.y * nq + qi;
    int64_t pos = 0, end = 0;
    if (FILL) {
        pos = offsets[qi] + part[slot];
        end = blockIdx.y + 1 < gridDim.y ? offsets[qi] + part[slot + nq] : offsets[qi + 1];
        if (end <= pos) return;
    }
    const int m0 = (int)blockIdx.y * per_range;
    const int m1 = (int)min((int64_t)nc, (int64_t)m0 + per_range);
    int cnt = 0;
    for (int m = m0; m < m1; ++m) {
        if (m == ex) continue;
        const uint8_t* cr = c + (size_t)m * nbytes;
        uint32_t inter = 0;
        for (int64_t j = lane; j < nbytes; j += 64) inter += __popc((uint32_t)(qr[j] & cr[j]));
        inter = wave_sum_u32(inter);
        const uint32_t un = qc + ccard[m] - inter;
        if (!(jaccard_dist(inter, un) <= radius)) continue;
        if (FILL) {
            if (lane == 0 && pos < end) {
                out_idx[pos] = m;
                if (out_inter) out_inter[pos] = inter;
                if (out_union) out_union[pos] = un;
            }
            ++pos;
        } else {
            ++cnt;
        }
    }
    if (!FILL && lane == 0) part[slot] = cnt;
}

__device__ __forceinline__ int wave_incl_scan_i32(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// One wave per query: part[r][q] (counts) -> the exclusive prefix over r, in place; offsets[q + 1] = the query's hits.
// (A query has at most nc < 2^31 hits: 32 bits hold every prefix.)
__global__ __launch_bounds__(256) void k_radius_sum(int64_t nq, int nsplit, int* __restrict__ part,
                                                    int64_t* __restrict__ offsets) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    int carry = 0;
    for (int r0 = 0; r0 < nsplit; r0 += 64) {
        const int r = r0 + lane;
        const int v = r < nsplit ? part[(int64_t)r * nq + qi] : 0;
        const int incl = wave_incl_scan_i32(v, lane);
        if (r < nsplit) part[(int64_t)r * nq + qi] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) offsets[qi + 1] = carry;
}

// One workgroup: the inclusive scan of offsets[1 .. nq] in place, 1024 entries a turn with a running carry; offsets[0] = 0
// and the total.  nq is a slab of queries, a few hundred turns of a microsecond at the most.
__global__ __launch_bounds__(1024) void k_radius_scan(int64_t nq, int64_t* __restrict__ offsets,
                                                      int64_t* __restrict__ total) {
    __shared__ long long wsum[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    for (int64_t base = 0; base < nq; base += 1024) {
        const int64_t i = base + tid;
        long long v = i < nq ? offsets[1 + i] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const long long t = wsum[w];
            before += w < wave ? t : 0;
            all += t;
        }
        if (i < nq) offsets[1 + i] = carry + before + v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        offsets[0] = 0;
        *total = carry;
    }
}

}  // namespace

extern "C" int bbh_jt_radius(const uint8_t* queries, int64_t nq, int64_t q_stride, const uint8_t* rows, int64_t nc,
                             int64_t nbytes, double radius, const int32_t* exclude, int64_t capacity,
                             int64_t* out_offsets, int64_t* out_total, int32_t* out_idx, uint32_t* out_inter,
                             uint32_t* out_union, void* stream) {
    BB_TRY(bb::ensure_device());
    if (nq < 0 || nc < 1 || nc > 0x7fffffffLL || nbytes <= 0 || q_stride < nbytes || out_offsets == nullptr ||
        out_total == nullptr)
        return bb::fail(BBH_ERR_INVALID,
                        "radius: need nq >= 0, 1 <= nc < 2^31, q_stride >= nbytes, an offsets and a total output");
    if (radius != radius) return bb::fail(BBH_ERR_INVALID, "radius: the radius is NaN");
    if (capacity < 0 || (capacity > 0 && out_idx == nullptr))
        return bb::fail(BBH_ERR_INVALID, "radius: need capacity >= 0, and an index output where capacity > 0");
    hipStream_t s = (hipStream_t)stream;
    bb::DevIn q, c, ex;
    bb::DevOut oo, ot, oi, on, ou;
    BB_TRY(oo.init(out_offsets, (size_t)(nq + 1) * 8));
    BB_TRY(ot.init(out_total, 8));
    bb::DevScope tmp(s);
    if (nq == 0) {
        BB_HIP(hipMemsetAsync(oo.dev, 0, 8, s));
        BB_HIP(hipMemsetAsync(ot.dev, 0, 8, s));
        BB_TRY(oo.finish(s));
        BB_TRY(ot.finish(s));
        return tmp.sync();
    }
    BB_TRY(q.init(queries, (size_t)((nq - 1) * q_stride + nbytes), s));
    BB_TRY(c.init(rows, (size_t)(nc * nbytes), s));
    BB_TRY(ex.init(exclude, (size_t)nq * 4, s));
    const uint8_t* qd = (const uint8_t*)q.dev;
    const uint8_t* cd = (const uint8_t*)c.dev;
    const int32_t* exd = (const int32_t*)ex.dev;
    int64_t* offd = (int64_t*)oo.dev;

    const bool al4 = (uintptr_t)qd % 4 == 0 && (uintptr_t)cd % 4 == 0 && q_stride % 4 == 0;
    const bool fast = al4 && radius_fast_width(nbytes);

    uint32_t* ccard = nullptr;
    BB_HIP(tmp.get(&ccard, (size_t)nc * 4));
    BB_TRY(bbh_popcount_rows(cd, nc, nbytes, nbytes, ccard, s));
    int64_t total = 0;
    {
        bb::ProfScope ps("jt_radius", s);
        ps.units(nq);
        int64_t qblocks = 0;
        int per = 0, nsplit = 0;
        radius_ranges(nq, nc, fast, 4, &qblocks, &per, &nsplit);
        int* part = nullptr;
        uint16_t* tab = nullptr;
        BB_HIP(tmp.get(&part, (size_t)nsplit * nq * 4));
        if (fast) {
            const int nbits = (int)nbytes * 8;
            BB_HIP(tmp.get(&tab, (size_t)(nbits + 1) * 2));
            hipLaunchKernelGGL(k_radius_table, dim3((unsigned)(nbits / 256 + 1)), dim3(256), 0, s, radius, nbits, tab);
            BB_HIP(hipGetLastError());
        }
        const dim3 grid((unsigned)qblocks, (unsigned)nsplit);
        int32_t* di = nullptr;
        uint32_t *dn = nullptr, *du = nullptr;
#define BB_LAUNCH_RADIUS(W, FILL)                                                                                     \
    hipLaunchKernelGGL((k_radius_bcnt<W, FILL>), grid, dim3(256), 0, s, qd, nq, q_stride, (const uint32_t*)cd, (int)nc, \
                       per, ccard, tab, exd, part, offd, di, dn, du)
#define BB_LAUNCH_RADIUS_PASS(FILL)                                                                                 \
    do {                                                                                                            \
        if (!fast)                                                                                                  \
            hipLaunchKernelGGL(k_radius_generic<FILL>, grid, dim3(256), 0, s, qd, nq, q_stride, cd, (int)nc, per,   \
                               nbytes, ccard, radius, exd, part, offd, di, dn, du);                                 \
        else if (nbytes == 8) BB_LAUNCH_RADIUS(2, FILL);                                                            \
        else if (nbytes == 16) BB_LAUNCH_RADIUS(4, FILL);                                                           \
        else if (nbytes == 32) BB_LAUNCH_RADIUS(8, FILL);                                                           \
        else if (nbytes == 64) BB_LAUNCH_RADIUS(16, FILL);                                                          \
        else if (nbytes == 128) BB_LAUNCH_RADIUS(32, FILL);                                                         \
        else BB_LAUNCH_RADIUS(64, FILL);                                                                            \
        BB_HIP(hipGetLastError());                                                                                  \
    } while (0)
        BB_LAUNCH_RADIUS_PASS(false);
        hipLaunchKernelGGL(k_radius_sum, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, nq, nsplit, part, offd);
        BB_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_radius_scan, dim3(1), dim3(1024), 0, s, nq, offd, (int64_t*)ot.dev);
        BB_HIP(hipGetLastError());
        // the host decides between filling and leaving: the one synchronisation in the middle of the call
        BB_HIP(hipMemcpyAsync(&total, ot.dev, 8, hipMemcpyDeviceToHost, s));
        BB_TRY(tmp.sync());
        if (total > 0 && total <= capacity) {
            BB_TRY(oi.init(out_idx, (size_t)total * 4));
            BB_TRY(on.init(out_inter, (size_t)total * 4));
            BB_TRY(ou.init(out_union, (size_t)total * 4));
            di = (int32_t*)oi.dev;
            dn = (uint32_t*)on.dev;
            du = (uint32_t*)ou.dev;
            BB_LAUNCH_RADIUS_PASS(true);
        }
#undef BB_LAUNCH_RADIUS_PASS
#undef BB_LAUNCH_RADIUS
    }
    BB_TRY(oo.finish(s));
    BB_TRY(ot.finish(s));
    BB_TRY(oi.finish(s));
    BB_TRY(on.finish(s));
    BB_TRY(ou.finish(s));
    return tmp.sync();
}
