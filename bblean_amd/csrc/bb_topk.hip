// bb_topk.hip -- the k nearest rows of a table for every query, for gfx950 (MI355X, CDNA4): what lies between
// bbh_jt_assign (the one nearest) and bbh_jt_dist_matrix (all of them), in nq x k memory.  DESIGN.md section 5e.
//
//   bbh_jt_topk        the k best candidates of every query, best first
//     k_topk_bcnt      AND + popcount, lane per query, for the usual widths (k_assign_bcnt's inner loop); the lane's
//                      list lives in LDS, only its worst entry in registers
//     k_topk_generic   every other width and alignment: one wave per query, the list one entry per lane
//     k_topk_combine   exact merge of the lists of the table ranges the grid was split into
//
// Order of two candidates (i, u, index) of one query: bb_assign.hip's.  A candidate is (n, u) with
// n = i + (u == 0);  a is better than b  <=>  n_a * u_b > n_b * u_a  (or equal and index_a < index_b); an empty
// union is (1, 0) and beats everything, "no candidate" is (-1, 1) and loses to everything.  Inside one range the
// index ascends, so a producer inserts on the strict product comparison alone; the combine compares the index too.
#include "bb_common.h"

using namespace bbd;

namespace {

constexpr int NO_IDX = 0x7fffffff;  // index of "no candidate" in a partial list

__device__ __forceinline__ bool better(long long an, long long au, int ai, long long bn, long long bu, int bi) {
    const long long l = an * bu, r = bn * au;
    return l > r || (l == r && ai < bi);
}

// (n, u) of rows of at most 2048 bits in one word: n + 1 in 0 .. 2050 above u in 0 .. 4096
__device__ __forceinline__ uint32_t pack_nu(int n, int u) { return ((uint32_t)(n + 1) << 16) | (uint32_t)u; }
__device__ __forceinline__ int packed_n(uint32_t p) { return (int)(p >> 16) - 1; }
__device__ __forceinline__ int packed_u(uint32_t p) { return (int)(p & 0xffffu); }

// ---------------------------------------------------------------------------------------------------------------
// AND + popcount.  Every lane owns one query row in registers; table rows are wave-uniform (scalar loads).  Grid:
// x = query tiles of blockDim.x, y = table ranges.
//
// Selection.  A lane's list is k (key, index) pairs in LDS, laid out [entry][lane] so that the lanes of a wave hit
// different banks whatever entries they are at.  It is NOT kept sorted: the lane knows where its worst entry is and
// holds that entry's (n, u) in registers as the threshold.  A row that beats the threshold strictly (the index ascends
// inside a range, so an equal fraction stays out) is appended to the lane's buffer of TOPK_BUF pairs, also in LDS;
// when any lane's buffer is full the whole wave works its buffers off: a candidate that still beats the worst entry
// replaces it, and the lane finds its new worst entry in one pass over the list - k independent LDS reads, not a
// chain of dependent shifts.  The buffer is what keeps the lanes together: a wave of 64 lanes meets a passing row
// almost every row until m >> 64 k, and without it every such row would cost the wave a pass over a list.
// ---------------------------------------------------------------------------------------------------------------
constexpr int TOPK_BUF = 8;

__device__ __forceinline__ void topk_flush(uint2* list, const uint2* buf, int T, int k, int& cnt, int& tn, int& tu,
                                           int& wpos) {
    for (int j = 0; j < TOPK_BUF; ++j) {
        const bool act = j < cnt;
        if (!__any(act)) break;
        const uint2 c = buf[j * T];
        const int cn = packed_n(c.x), cu = packed_u(c.x);
        const bool pass = act && __mul24(cn, tu) > __mul24(tn, cu);
        if (!__any(pass)) continue;
        if (pass) list[wpos * T] = c;
        uint2 w = list[0];
        int wp = 0;
        for (int t = 1; t < k; ++t) {  // the worst entry: the smallest fraction, the larger index among equal ones
            const uint2 e = list[t * T];
            const int l = __mul24(packed_n(e.x), packed_u(w.x)), r = __mul24(packed_n(w.x), packed_u(e.x));
            if (l < r || (l == r && (int)e.y > (int)w.y)) {
                w = e;
                wp = t;
            }
        }
        wpos = wp;
        tn = packed_n(w.x);
        tu = packed_u(w.x);
    }
    cnt = 0;
}

template <int W32>
__global__ __launch_bounds__(256) void k_topk_bcnt(const uint8_t* __restrict__ q, int64_t nq, int64_t q_stride,
                                                   const uint32_t* __restrict__ c, int nc, int per_range,
                                                   const uint32_t* __restrict__ ccard, int k,
                                                   const int32_t* __restrict__ exclude, int* __restrict__ part_n,
                                                   int* __restrict__ part_u, int* __restrict__ part_idx,
                                                   int32_t* __restrict__ out_idx, uint32_t* __restrict__ out_inter,
                                                   uint32_t* __restrict__ out_union) {
    extern __shared__ __attribute__((aligned(16))) uint2 lds[];
    const int T = (int)blockDim.x, tid = (int)threadIdx.x;
    uint2* list = lds + tid;         // list[j * T], j < k
    uint2* buf = lds + k * T + tid;  // buf[j * T], j < TOPK_BUF
    const int64_t qi = (int64_t)blockIdx.x * T + tid;
    const bool ok = qi < nq;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(q + (ok ? qi : 0) * q_stride);
    uint32_t x[W32];
    uint32_t qc = 0;
#pragma unroll
    for (int w = 0; w < W32; ++w) {
        x[w] = ok ? src[w] : 0u;
        qc += __popc(x[w]);
    }
    // "no candidate" everywhere; a lane without a query holds (1, 0) everywhere: nothing ever beats its threshold
    int tn = ok ? -1 : 1, tu = ok ? 1 : 0, wpos = 0, cnt = 0;
    for (int j = 0; j < k; ++j) list[j * T] = make_uint2(pack_nu(tn, tu), (uint32_t)NO_IDX);
    const int ex = (ok && exclude != nullptr) ? exclude[qi] : -1;
    const int m0 = (int)blockIdx.y * per_range;
    const int m1 = (int)min((int64_t)nc, (int64_t)m0 + per_range);
    for (int m = m0; m < m1; ++m) {
        const uint32_t* cr = c + (size_t)m * W32;  // wave-uniform address
        uint32_t inter = 0;
#pragma unroll
        for (int w = 0; w < W32; ++w) inter += __popc(x[w] & cr[w]);
        const int un = (int)(qc + ccard[m] - inter);
        const int n = (int)inter + (un == 0 ? 1 : 0);
        // (__mul24: n <= 2049 and u <= 4096 fit its 24 bits, -1 included, and the products fit the 32 it returns)
        if (__mul24(n, tu) > __mul24(tn, un) && m != ex) {
            buf[cnt * T] = make_uint2(pack_nu(n, un), (uint32_t)m);
            ++cnt;
        }
        if (__any(cnt == TOPK_BUF)) topk_flush(list, buf, T, k, cnt, tn, tu, wpos);
    }
    topk_flush(list, buf, T, k, cnt, tn, tu, wpos);
    if (!ok) return;
    if (out_idx != nullptr) {  // one range: the list, sorted by selection, is the result
        for (int j = 0; j < k; ++j) {
            uint2 b = list[j * T];
            int bp = j;
            for (int t = j + 1; t < k; ++t) {
                const uint2 e = list[t * T];
                const int l = __mul24(packed_n(e.x), packed_u(b.x)), r = __mul24(packed_n(b.x), packed_u(e.x));
                if (l > r || (l == r && (int)e.y < (int)b.y)) {
                    b = e;
                    bp = t;
                }
            }
            if (bp != j) list[bp * T] = list[j * T];
            const int64_t o = qi * k + j;
            out_idx[o] = (int)b.y;
            if (out_inter) out_inter[o] = packed_u(b.x) == 0 ? 0u : (uint32_t)packed_n(b.x);
            if (out_union) out_union[o] = (uint32_t)packed_u(b.x);
        }
        return;
    }
    const int64_t o0 = ((int64_t)blockIdx.y * nq + qi) * k;  // (in the list's order: the combine does not need it sorted)
    for (int j = 0; j < k; ++j) {
        const uint2 e = list[j * T];
        part_n[o0 + j] = packed_n(e.x);
        part_u[o0 + j] = packed_u(e.x);
        part_idx[o0 + j] = (int)e.y;
    }
}

// A wave's sorted list, entry j in lane j (lanes >= k stay out): the wave-uniform candidate goes in before the first
// entry it beats, the entries from there on move one lane up and the last one falls off.
__device__ __forceinline__ void wave_list_insert(int lane, int k, bool full_order, long long cn, long long cu, int ci,
                                                 long long& ln, long long& lu, int& li) {
    const bool beats = lane < k && (full_order ? better(cn, cu, ci, ln, lu, li) : cn * lu > ln * cu);
    const unsigned long long mask = __ballot(beats);
    if (mask == 0ull) return;
    const int pos = __ffsll((long long)mask) - 1;
    const long long pn = __shfl_up(ln, 1), pu = __shfl_up(lu, 1);
    const int pi = __shfl_up(li, 1);
    if (lane == pos) {
        ln = cn;
        lu = cu;
        li = ci;
    } else if (lane > pos) {
        ln = pn;
        lu = pu;
        li = pi;
    }
}

// any width, any alignment: one wave per query, lanes stride over the bytes of every row of the range
__global__ __launch_bounds__(256) void k_topk_generic(const uint8_t* __restrict__ q, int64_t nq, int64_t q_stride,
                                                      const uint8_t* __restrict__ c, int nc, int per_range,
                                                      int64_t nbytes, const uint32_t* __restrict__ ccard, int k,
                                                      const int32_t* __restrict__ exclude, int* __restrict__ part_n,
                                                      int* __restrict__ part_u, int* __restrict__ part_idx) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const uint8_t* qr = q + qi * q_stride;
    uint32_t qc = 0;
    for (int64_t j = lane; j < nbytes; j += 64) qc += __popc((uint32_t)qr[j]);
    qc = wave_sum_u32(qc);
    const int ex = exclude != nullptr ? exclude[qi] : -1;
    const int m0 = (int)blockIdx.y * per_range;
    const int m1 = (int)min((int64_t)nc, (int64_t)m0 + per_range);
    long long ln = -1, lu = 1;
    int li = NO_IDX;
    for (int m = m0; m < m1; ++m) {
        if (m == ex) continue;
        const uint8_t* cr = c + (size_t)m * nbytes;
        uint32_t inter = 0;
        for (int64_t j = lane; j < nbytes; j += 64) inter += __popc((uint32_t)(qr[j] & cr[j]));
        inter = wave_sum_u32(inter);
        const long long un = (long long)qc + ccard[m] - inter;
        const long long n = (long long)inter + (un == 0 ? 1 : 0);
        wave_list_insert(lane, k, false, n, un, m, ln, lu, li);
    }
    if (lane < k) {
        const int64_t o = ((int64_t)blockIdx.y * nq + qi) * k + lane;
        part_n[o] = (int)ln;
        part_u[o] = (int)lu;
        part_idx[o] = li;
    }
}

// the lists of the ranges (in any order) -> the result (exact: 64-bit cross-multiplication, lowest index on ties).  One wave
// per query; 64 entries of the partial lists at a time are held against the k-th best so far, and the few that beat it
// go into the wave's list one by one.
__global__ __launch_bounds__(256) void k_topk_combine(int64_t nq, int nsplit, int k, const int* __restrict__ part_n,
                                                      const int* __restrict__ part_u, const int* __restrict__ part_idx,
                                                      int32_t* __restrict__ out_idx, uint32_t* __restrict__ out_inter,
                                                      uint32_t* __restrict__ out_union) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    long long ln = -1, lu = 1;
    int li = NO_IDX;
    const int64_t total = (int64_t)nsplit * k;
    for (int64_t e0 = 0; e0 < total; e0 += 64) {
        const int64_t e = e0 + lane;
        long long cn = -1, cu = 1;
        int ci = NO_IDX;
        if (e < total) {
            const int64_t o = ((e / k) * nq + qi) * k + e % k;
            cn = part_n[o];
            cu = part_u[o];
            ci = part_idx[o];
        }
        const long long tn = __shfl(ln, k - 1), tu = __shfl(lu, k - 1);
        const int ti = __shfl(li, k - 1);
        unsigned long long pass = __ballot(cn >= 0 && better(cn, cu, ci, tn, tu, ti));
        while (pass != 0ull) {
            const int b = __ffsll((long long)pass) - 1;
            pass &= pass - 1;
            wave_list_insert(lane, k, true, __shfl(cn, b), __shfl(cu, b), __shfl(ci, b), ln, lu, li);
        }
    }
    if (lane < k) {
        const int64_t o = qi * k + lane;
        out_idx[o] = li;
        if (out_inter) out_inter[o] = lu == 0 ? 0u : (uint32_t)ln;
        if (out_union) out_union[o] = (uint32_t)lu;
    }
}

int cu_count() {
    static int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;
        return v;
    }();
    return n;
}

// lanes of a k_topk_bcnt workgroup: (k + TOPK_BUF) pairs of 8 bytes per lane, at most 36 KiB of LDS per workgroup
int topk_block(int k) { return k <= 8 ? 256 : k <= 24 ? 128 : 64; }

}  // namespace

extern "C" int bbh_jt_topk(const uint8_t* queries, int64_t nq, int64_t q_stride, const uint8_t* rows, int64_t nc,
                           int64_t nbytes, int32_t k, const int32_t* exclude, int32_t* out_idx, uint32_t* out_inter,
                           uint32_t* out_union, void* stream) {
    BB_TRY(bb::ensure_device());
    if (nq < 0 || nc < 1 || nc > 0x7fffffffLL || nbytes <= 0 || q_stride < nbytes || out_idx == nullptr)
        return bb::fail(BBH_ERR_INVALID, "topk: need nq >= 0, 1 <= nc < 2^31, q_stride >= nbytes and an index output");
    if (k < 1 || k > BBH_TOPK_MAX || k > nc - (exclude != nullptr ? 1 : 0))
        return bb::fail(BBH_ERR_INVALID, "topk: need 1 <= k <= BBH_TOPK_MAX (%d) and k <= nc (nc - 1 with exclude)",
                        BBH_TOPK_MAX);
    if (nq == 0) return BBH_OK;
    hipStream_t s = (hipStream_t)stream;
    bb::DevIn q, c, ex;
    bb::DevOut oi, on, ou;
    BB_TRY(q.init(queries, (size_t)((nq - 1) * q_stride + nbytes), s));
    BB_TRY(c.init(rows, (size_t)(nc * nbytes), s));
    BB_TRY(ex.init(exclude, (size_t)nq * 4, s));
    BB_TRY(oi.init(out_idx, (size_t)nq * k * 4));
    BB_TRY(on.init(out_inter, (size_t)nq * k * 4));
    BB_TRY(ou.init(out_union, (size_t)nq * k * 4));
    const uint8_t* qd = (const uint8_t*)q.dev;
    const uint8_t* cd = (const uint8_t*)c.dev;
    const int32_t* exd = (const int32_t*)ex.dev;

    const bool al4 = (uintptr_t)qd % 4 == 0 && (uintptr_t)cd % 4 == 0 && q_stride % 4 == 0;
    const bool fast = al4 && (nbytes == 8 || nbytes == 16 || nbytes == 32 || nbytes == 64 || nbytes == 128 ||
                              nbytes == 256);
    const int T = topk_block(k);

    bb::DevScope tmp(s);
    uint32_t* ccard = nullptr;
    BB_HIP(tmp.get(&ccard, (size_t)nc * 4));
    BB_TRY(bbh_popcount_rows(cd, nc, nbytes, nbytes, ccard, s));
    {
        bb::ProfScope ps("jt_topk", s);
        ps.units(nq);
        // the ranges of bbh_jt_assign: fill the device four times over, with at least 64 rows per range.  Workgroups of 128
        // lanes count as halves, so that they bring as many waves; those of 64 lanes (k > 24) do not: LDS admits four or
        // five of them per CU whatever the grid, and shorter ranges only add replacements
        const int64_t qblocks = fast ? (nq + T - 1) / T : (nq + 3) / 4;
        const int64_t fill = 4 * (int64_t)cu_count() * (fast && T == 128 ? 2 : 1);
        int64_t want = (fill + qblocks - 1) / qblocks;
        const int64_t most = (nc + 63) / 64;
        if (want > most) want = most;
        if (want > 65535) want = 65535;
        const int per = (int)((nc + want - 1) / want);
        const int nsplit = (int)((nc + per - 1) / per);
        const bool direct = fast && nsplit == 1;  // the producer writes the result itself
        int *pn = nullptr, *pu = nullptr, *pi = nullptr;
        if (!direct) {
            BB_HIP(tmp.get(&pn, (size_t)nsplit * nq * k * 4));
            BB_HIP(tmp.get(&pu, (size_t)nsplit * nq * k * 4));
            BB_HIP(tmp.get(&pi, (size_t)nsplit * nq * k * 4));
        }
        const dim3 grid((unsigned)qblocks, (unsigned)nsplit);
        int32_t* di = direct ? (int32_t*)oi.dev : nullptr;
        uint32_t* dn = direct ? (uint32_t*)on.dev : nullptr;
        uint32_t* du = direct ? (uint32_t*)ou.dev : nullptr;
#define BB_LAUNCH_TOPK(W)                                                                                        \
    hipLaunchKernelGGL((k_topk_bcnt<W>), grid, dim3(T), (size_t)(k + TOPK_BUF) * T * 8, s, qd, nq, q_stride, (const uint32_t*)cd, \
                       (int)nc, per, ccard, (int)k, exd, pn, pu, pi, di, dn, du)
        if (!fast)
            hipLaunchKernelGGL(k_topk_generic, grid, dim3(256), 0, s, qd, nq, q_stride, cd, (int)nc, per, nbytes, ccard,
                               (int)k, exd, pn, pu, pi);
        else if (nbytes == 8) BB_LAUNCH_TOPK(2);
        else if (nbytes == 16) BB_LAUNCH_TOPK(4);
        else if (nbytes == 32) BB_LAUNCH_TOPK(8);
        else if (nbytes == 64) BB_LAUNCH_TOPK(16);
        else if (nbytes == 128) BB_LAUNCH_TOPK(32);
        else BB_LAUNCH_TOPK(64);
#undef BB_LAUNCH_TOPK
        BB_HIP(hipGetLastError());
        if (!direct) {
            hipLaunchKernelGGL(k_topk_combine, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, nq, nsplit, (int)k, pn, pu,
                               pi, (int32_t*)oi.dev, (uint32_t*)on.dev, (uint32_t*)ou.dev);
            BB_HIP(hipGetLastError());
        }
    }
    BB_TRY(oi.finish(s));
    BB_TRY(on.finish(s));
    BB_TRY(ou.finish(s));
    return tmp.sync();
}
