// bb_assign.hip -- assignment of new fingerprints to fitted clusters (sklearn.BitBirch.predict / .transform of the
// reference, bblean/sklearn.py:123-153) for gfx950 (MI355X, CDNA4).
//
//   bbh_jt_assign       nearest centroid of every query: first index of the minimum Jaccard distance
//     k_assign_mfma     2048-bit rows: intersection counts on the int8 matrix cores (v_mfma_i32_16x16x64_i8)
//     k_assign_bcnt     AND + popcount, lane per query, for the usual widths; k_assign_generic for every other
//     k_assign_combine  exact combine of the winners of the centroid ranges the grid was split into
//   bbh_jt_dist_matrix  the nq x nc float64 matrix of (u - i) / u
//
// Ordering of two candidates (i, u, index) of one query, shared by every kernel here.  The reference takes the
// first minimum of d = (u - i) / u with d = 0 where u == 0, i.e. an empty union beats everything, then the larger
// i / u, then the smaller index.  A candidate is held as (n, u) with n = i + (u == 0): then
//        a is better than b  <=>  n_a * u_b > n_b * u_a   (or equal and index_a < index_b)
// is that order in plain integers: an empty union is (1, 0), which beats every (n, u >= 1) because u > 0 and loses
// to nothing because n * 0 > u never holds; "no candidate yet" is (-1, 1), which loses to everything.
#include "bb_common.h"

#include <cstdlib>

using namespace bbd;

namespace {

struct Cand {
    int n, u, idx;
};

__device__ __forceinline__ bool better(long long an, long long au, int ai, long long bn, long long bu, int bi) {
    const long long l = an * bu, r = bn * au;
    return l > r || (l == r && ai < bi);
}

// ---------------------------------------------------------------------------------------------------------------
// AND + popcount.  Every lane owns one query row in registers; centroid rows are wave-uniform (scalar loads), as
// in k_best_match.  Grid: x = query tiles of 256, y = centroid ranges; range y writes its winners to part[y].
// ---------------------------------------------------------------------------------------------------------------
template <int W32>
__global__ __launch_bounds__(256) void k_assign_bcnt(const uint8_t* __restrict__ q, int64_t nq, int64_t q_stride,
                                                     const uint32_t* __restrict__ c, int nc, int per_range,
                                                     const uint32_t* __restrict__ ccard, int* __restrict__ part_n,
                                                     int* __restrict__ part_u, int* __restrict__ part_idx) {
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = qi < nq;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(q + (ok ? qi : 0) * q_stride);
    uint32_t x[W32];
    uint32_t qc = 0;
#pragma unroll
    for (int w = 0; w < W32; ++w) {
        x[w] = ok ? src[w] : 0u;
        qc += __popc(x[w]);
    }
    const int m0 = (int)blockIdx.y * per_range;
    const int m1 = (int)min((int64_t)nc, (int64_t)m0 + per_range);
    int bn = -1, bu = 1, best = m0;
    for (int m = m0; m < m1; ++m) {
        const uint32_t* cr = c + (size_t)m * W32;  // wave-uniform address
        uint32_t inter = 0;
#pragma unroll
        for (int w = 0; w < W32; ++w) inter += __popc(x[w] & cr[w]);
        const int un = (int)(qc + ccard[m] - inter);
        const int n = (int)inter + (un == 0 ? 1 : 0);
        if (n * bu > bn * un) {  // strict: the first index of equal fractions stays (products <= 2^23 for W32 <= 64)
            bn = n;
            bu = un;
            best = m;
        }
    }
    if (ok) {
        const int64_t o = (int64_t)blockIdx.y * nq + qi;
        part_n[o] = bn;
        part_u[o] = bu;
        part_idx[o] = best;
    }
}

// any width, any alignment: one wave per query, lanes stride over the bytes of every centroid of the range
__global__ __launch_bounds__(256) void k_assign_generic(const uint8_t* __restrict__ q, int64_t nq, int64_t q_stride,
                                                        const uint8_t* __restrict__ c, int nc, int per_range,
                                                        int64_t nbytes, const uint32_t* __restrict__ ccard,
                                                        int* __restrict__ part_n, int* __restrict__ part_u,
                                                        int* __restrict__ part_idx) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const uint8_t* qr = q + qi * q_stride;
    uint32_t qc = 0;
    for (int64_t j = lane; j < nbytes; j += 64) qc += __popc((uint32_t)qr[j]);
    qc = wave_sum_u32(qc);
    const int m0 = (int)blockIdx.y * per_range;
    const int m1 = (int)min((int64_t)nc, (int64_t)m0 + per_range);
    long long bn = -1, bu = 1;
    int best = m0;
    for (int m = m0; m < m1; ++m) {
        const uint8_t* cr = c + (size_t)m * nbytes;
        uint32_t inter = 0;
        for (int64_t j = lane; j < nbytes; j += 64) inter += __popc((uint32_t)(qr[j] & cr[j]));
        inter = wave_sum_u32(inter);
        const long long un = (long long)qc + ccard[m] - inter;
        const long long n = (long long)inter + (un == 0 ? 1 : 0);
        if (n * bu > bn * un) {
            bn = n;
            bu = un;
            best = m;
        }
    }
    if (lane == 0) {
        const int64_t o = (int64_t)blockIdx.y * nq + qi;
        part_n[o] = (int)bn;
        part_u[o] = (int)bu;
        part_idx[o] = best;
    }
}

// winners of the centroid ranges -> the result (exact: 64-bit cross-multiplication, lowest index on ties)
__global__ __launch_bounds__(256) void k_assign_combine(int64_t nq, int nsplit, const int* __restrict__ part_n,
                                                        const int* __restrict__ part_u, const int* __restrict__ part_idx,
                                                        int32_t* __restrict__ out_idx, uint32_t* __restrict__ out_inter,
                                                        uint32_t* __restrict__ out_union) {
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    long long bn = part_n[qi], bu = part_u[qi];
    int best = part_idx[qi];
    for (int s = 1; s < nsplit; ++s) {
        const int64_t o = (int64_t)s * nq + qi;
        const long long n = part_n[o], u = part_u[o];
        const int idx = part_idx[o];
        if (better(n, u, idx, bn, bu, best)) {
            bn = n;
            bu = u;
            best = idx;
        }
    }
    out_idx[qi] = best;
    if (out_inter) out_inter[qi] = bu == 0 ? 0u : (uint32_t)bn;
    if (out_union) out_union[qi] = (uint32_t)bu;
}

// ---------------------------------------------------------------------------------------------------------------
// int8 matrix cores, 2048-bit rows.  A workgroup (4 waves) owns 128 queries and walks centroid tiles of 128 rows; per
// K-chunk of 256 bits both operands are expanded from packed bits to 0/1 bytes in LDS (128 rows x 256 B each) and
// every wave runs 4 x 4 tiles of v_mfma_i32_16x16x64_i8 on its 64 x 64 part: centroids are the A operand (rows of
// the accumulator: row = 4 * (lane >> 4) + reg), queries the B operand (col = lane & 15), so a lane's registers
// hold candidates of ONE query per column tile and the per-query reduction is a scan of the lane's own registers;
// the four lanes and two waves that share a query meet once, after the last tile.
//
// Expansion: dword j (0..7) of the 32 bytes a 32-bit word w expands to is (w >> j) & 0x01010101, i.e. bits j, j + 8,
// j + 16, j + 24 - two VALU operations per 4 bytes.  That is NOT bit order, and it need not be: a dot product
// does not care in which order K is summed as long as both operands use the same one, and they share this code.
// The same holds for which 16 bytes of the K-step a lane group holds (see the probe k_mfma_i8_probe for the map).
//
// LDS image of one operand chunk: row r at r * 256 B, its 16-byte slot s (0..15) stored at slot s ^ (r & 15): a
// fragment read (16 rows x 4 slots per ds_read_b128) and the expansion's 16-byte stores then touch every bank once.
// ---------------------------------------------------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int TQ = 128, TC = 128, KCH = 8;  // 8 K-chunks of 256 bits
constexpr int CC_PAD = 4096;                // popcount given to the rows behind the last centroid: they lose or tie with a higher index

__device__ __forceinline__ void expand_store(uint8_t* lds, int row, int half, uint4 v) {
    // this thread's 128 bits -> 128 bytes = slots half * 8 .. half * 8 + 7 of `row`
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint8_t* base = lds + row * 256;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            uint4 o;
            o.x = (w[i] >> (4 * s + 0)) & 0x01010101u;
            o.y = (w[i] >> (4 * s + 1)) & 0x01010101u;
            o.z = (w[i] >> (4 * s + 2)) & 0x01010101u;
            o.w = (w[i] >> (4 * s + 3)) & 0x01010101u;
            const int slot = (half * 8 + 2 * i + s) ^ (row & 15);
            *reinterpret_cast<uint4*>(base + slot * 16) = o;
        }
    }
}

__device__ __forceinline__ v4i frag_load(const uint8_t* lds, int row, int slot) {
    return *reinterpret_cast<const v4i*>(lds + row * 256 + ((slot ^ (row & 15)) * 16));
}

__global__ __launch_bounds__(256) void k_assign_mfma(const uint8_t* __restrict__ q, int64_t nq, int64_t q_stride,
                                                     const uint8_t* __restrict__ c, int nc, int tiles_per_range,
                                                     const uint32_t* __restrict__ qcard,
                                                     const uint32_t* __restrict__ ccard, int* __restrict__ part_n,
                                                     int* __restrict__ part_u, int* __restrict__ part_idx) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_c[TC * 256];
    __shared__ __attribute__((aligned(16))) uint8_t lds_q[TQ * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int wc = (wave >> 1) * 64, wq = (wave & 1) * 64;  // this wave's 64 centroid rows x 64 query columns of the tile
    const int64_t q0 = (int64_t)blockIdx.x * TQ;
    const int n_tiles = (nc + TC - 1) / TC;
    const int t0 = (int)blockIdx.y * tiles_per_range;
    const int t1 = min(n_tiles, t0 + tiles_per_range);

    // staging: thread -> (row, half) of both operands; 16 bytes = half a chunk of one row
    const int srow = tid >> 1, shalf = tid & 1;
    const int64_t sq = q0 + srow;
    const uint8_t* qsrc = q + (sq < nq ? sq : 0) * q_stride + shalf * 16;
    const bool q_ok = sq < nq;

    int qc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int64_t col = q0 + wq + 16 * nt + l15;
        qc[nt] = col < nq ? (int)qcard[col] : 0;
    }
    Cand best[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) best[nt] = Cand{-1, 1, 0x7fffffff};

    for (int t = t0; t < t1; ++t) {
        const int c0 = t * TC;
        const bool c_ok = c0 + srow < nc;
        const uint8_t* csrc = c + (size_t)(c_ok ? c0 + srow : 0) * 256 + shalf * 16;
        v4i acc[4][4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = v4i{0, 0, 0, 0};
        uint4 vc = c_ok ? *reinterpret_cast<const uint4*>(csrc) : make_uint4(0, 0, 0, 0);
        uint4 vq = q_ok ? *reinterpret_cast<const uint4*>(qsrc) : make_uint4(0, 0, 0, 0);
        for (int k = 0; k < KCH; ++k) {
            __syncthreads();  // the previous chunk's fragments have been read
            expand_store(lds_c, srow, shalf, vc);
            expand_store(lds_q, srow, shalf, vq);
            __syncthreads();
            if (k + 1 < KCH) {  // next chunk's packed bits travel while this one is multiplied
                vc = c_ok ? *reinterpret_cast<const uint4*>(csrc + (k + 1) * 32) : make_uint4(0, 0, 0, 0);
                vq = q_ok ? *reinterpret_cast<const uint4*>(qsrc + (k + 1) * 32) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                v4i a[4], b[4];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) a[mt] = frag_load(lds_c, wc + 16 * mt + l15, 4 * ks + g);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) b[nt] = frag_load(lds_q, wq + 16 * nt + l15, 4 * ks + g);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
            }
        }
        // epilogue: this lane's 16 centroid rows (ascending index) against its 4 query columns
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = c0 + wc + 16 * mt + 4 * g + r;
                const int cc = m < nc ? (int)ccard[m] : CC_PAD;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const int inter = acc[mt][nt][r];
                    const int un = qc[nt] + cc - inter;
                    const int n = inter + (un == 0 ? 1 : 0);
                    // (__mul24 multiplies the low 24 bits of its operands, signed: n <= 2049 and u <= 6144 fit, -1 included;
                    //  the products, up to 2049 * 6144 < 2^24, fit the 32 bits it returns)
                    if (__mul24(n, best[nt].u) > __mul24(best[nt].n, un)) best[nt] = Cand{n, un, m};
                }
            }
        }
    }

    // the four lane groups of a column, then the two waves of a column (LDS is free again after the barrier)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int x = 16; x <= 32; x <<= 1) {
            const int on = __shfl_xor(best[nt].n, x), ou = __shfl_xor(best[nt].u, x), oi = __shfl_xor(best[nt].idx, x);
            if (better(on, ou, oi, best[nt].n, best[nt].u, best[nt].idx)) best[nt] = Cand{on, ou, oi};
        }
    }
    __syncthreads();
    int* xch = reinterpret_cast<int*>(lds_c);  // [2 centroid halves][128 queries][3]
    if (g == 0) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            int* p = xch + ((wave >> 1) * TQ + wq + 16 * nt + l15) * 3;
            p[0] = best[nt].n;
            p[1] = best[nt].u;
            p[2] = best[nt].idx;
        }
    }
    __syncthreads();
    if (tid < TQ && q0 + tid < nq) {
        const int* a = xch + tid * 3;
        const int* b = xch + (TQ + tid) * 3;
        const bool second = better(b[0], b[1], b[2], a[0], a[1], a[2]);
        const int* w = second ? b : a;
        const int64_t o = (int64_t)blockIdx.y * nq + q0 + tid;
        part_n[o] = w[0];
        part_u[o] = w[1];
        part_idx[o] = w[2];
    }
}

// The operand maps of v_mfma_i32_16x16x64_i8, established with exact integer data (tests/test_hip_assign.py):
// lane l holds A[row l & 15][k = 16 * (l >> 4) + j] and B[k = 16 * (l >> 4) + j][col l & 15] in byte j = 0..15 of its
// fragment; D[row 4 * (l >> 4) + reg][col l & 15].  One wave, one tile: a (16 x 64), b (64 x 16), d (16 x 16), row-major.
__global__ __launch_bounds__(64) void k_mfma_i8_probe(const int8_t* __restrict__ a, const int8_t* __restrict__ b,
                                                      int32_t* __restrict__ d) {
    const int lane = threadIdx.x, l15 = lane & 15, g = lane >> 4;
    union {
        v4i v;
        int8_t e[16];
    } fa, fb;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        fa.e[j] = a[l15 * 64 + 16 * g + j];
        fb.e[j] = b[(16 * g + j) * 16 + l15];
    }
    v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa.v, fb.v, v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) d[(4 * g + r) * 16 + l15] = acc[r];
}

// ---------------------------------------------------------------------------------------------------------------
// transform: out[q][m] = (u - i) / u as one float64 division of exact integers, 0.0 where u == 0.  Bound by its 8
// bytes of output per pair.  Here every lane owns one CENTROID row in registers and the query rows are the
// wave-uniform operand, so a wave writes 64 consecutive m of one query: 512 contiguous bytes.
// Grid: x = centroid tiles of 256, y = query ranges.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double jaccard_dist(uint32_t inter, uint32_t un) {
    return un == 0u ? 0.0 : (double)(un - inter) / (double)un;
}

template <int W32>
__global__ __launch_bounds__(256) void k_jaccard_dist(const uint8_t* __restrict__ q, int64_t nq, int64_t q_stride,
                                                      const uint32_t* __restrict__ c, int64_t nc, int64_t q_per_range,
                                                      const uint32_t* __restrict__ qcard, double* __restrict__ out) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = m < nc;
    const uint32_t* src = c + (ok ? m : 0) * W32;
    uint32_t x[W32];
    uint32_t cc = 0;
#pragma unroll
    for (int w = 0; w < W32; ++w) {
        x[w] = ok ? src[w] : 0u;
        cc += __popc(x[w]);
    }
    const int64_t qa = (int64_t)blockIdx.y * q_per_range;
    const int64_t qb = min(nq, qa + q_per_range);
    for (int64_t qi = qa; qi < qb; ++qi) {
        const uint32_t* qr = reinterpret_cast<const uint32_t*>(q + qi * q_stride);  // wave-uniform address
        uint32_t inter = 0;
#pragma unroll
        for (int w = 0; w < W32; ++w) inter += __popc(x[w] & qr[w]);
        if (ok) __builtin_nontemporal_store(jaccard_dist(inter, qcard[qi] + cc - inter), out + qi * nc + m);
    }
}

// any width, any alignment: one thread per pair, consecutive threads on consecutive m
__global__ __launch_bounds__(256) void k_jaccard_dist_generic(const uint8_t* __restrict__ q, int64_t nq,
                                                              int64_t q_stride, const uint8_t* __restrict__ c,
                                                              int64_t nc, int64_t nbytes, double* __restrict__ out) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t qi = blockIdx.y + (int64_t)blockIdx.z * 65535;
    if (m >= nc || qi >= nq) return;
    const uint8_t* qr = q + qi * q_stride;
    const uint8_t* cr = c + m * nbytes;
    uint32_t inter = 0, qc = 0, cc = 0;
    for (int64_t j = 0; j < nbytes; ++j) {
        const uint32_t a = qr[j], b = cr[j];
        inter += __popc(a & b);
        qc += __popc(a);
        cc += __popc(b);
    }
    out[qi * nc + m] = jaccard_dist(inter, qc + cc - inter);
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

// BBHIP_ASSIGN=bcnt|mfma forces a kernel; anything else (or unset) = the dispatch rule
int forced_kernel() {
    const char* e = getenv("BBHIP_ASSIGN");
    if (e == nullptr) return 0;
    if (std::strcmp(e, "bcnt") == 0) return 1;
    if (std::strcmp(e, "mfma") == 0) return 2;
    return 0;
}

}  // namespace

extern "C" int bbh_jt_assign(const uint8_t* queries, int64_t nq, int64_t q_stride, const uint8_t* cents, int64_t nc,
                             int64_t nbytes, int32_t* out_idx, uint32_t* out_inter, uint32_t* out_union,
                             void* stream) {
    BB_TRY(bb::ensure_device());
    if (nq < 0 || nc < 1 || nc > 0x7fffffffLL || nbytes <= 0 || q_stride < nbytes || out_idx == nullptr)
        return bb::fail(BBH_ERR_INVALID, "assign: need nq >= 0, 1 <= nc < 2^31, q_stride >= nbytes and an index output");
    if (nq == 0) return BBH_OK;
    hipStream_t s = (hipStream_t)stream;
    bb::DevIn q, c;
    bb::DevOut oi, on, ou;
    BB_TRY(q.init(queries, (size_t)((nq - 1) * q_stride + nbytes), s));
    BB_TRY(c.init(cents, (size_t)(nc * nbytes), s));
    BB_TRY(oi.init(out_idx, (size_t)nq * 4));
    BB_TRY(on.init(out_inter, (size_t)nq * 4));
    BB_TRY(ou.init(out_union, (size_t)nq * 4));
    const uint8_t* qd = (const uint8_t*)q.dev;
    const uint8_t* cd = (const uint8_t*)c.dev;

    const int forced = forced_kernel();
    const bool al16 = (uintptr_t)qd % 16 == 0 && (uintptr_t)cd % 16 == 0 && q_stride % 16 == 0;
    const bool al4 = (uintptr_t)qd % 4 == 0 && (uintptr_t)cd % 4 == 0 && q_stride % 4 == 0;
    const bool mfma_ok = nbytes == 256 && al16;
    if (forced == 2 && !mfma_ok)
        return bb::fail(BBH_ERR_INVALID, "assign: BBHIP_ASSIGN=mfma needs 256-byte rows at 16-byte aligned addresses");
    // dispatch rule: the matrix-core kernel for 2048-bit rows once a centroid tile is worth
    // filling, AND + popcount otherwise
    const bool use_mfma = forced == 2 || (forced == 0 && mfma_ok && nc >= 64 && nq >= 64);
    const int cus = cu_count();

    bb::DevScope tmp(s);
    uint32_t *ccard = nullptr, *qcard = nullptr;
    BB_HIP(tmp.get(&ccard, (size_t)nc * 4));
    BB_TRY(bbh_popcount_rows(cd, nc, nbytes, nbytes, ccard, s));
    int nsplit = 1;
    int *pn = nullptr, *pu = nullptr, *pi = nullptr;
    {
        bb::ProfScope ps("jt_assign", s);
        ps.units(nq);
        if (use_mfma) {
            BB_HIP(tmp.get(&qcard, (size_t)nq * 4));
            BB_TRY(bbh_popcount_rows(qd, nq, nbytes, q_stride, qcard, s));
            const int64_t qtiles = (nq + TQ - 1) / TQ;
            const int ctiles = (int)((nc + TC - 1) / TC);
            int64_t want = (2 * (int64_t)cus + qtiles - 1) / qtiles;  // two workgroups per CU
            if (want > ctiles) want = ctiles;
            if (want > 65535) want = 65535;
            const int per = (int)((ctiles + want - 1) / want);
            nsplit = (ctiles + per - 1) / per;
            BB_HIP(tmp.get(&pn, (size_t)nsplit * nq * 4));
            BB_HIP(tmp.get(&pu, (size_t)nsplit * nq * 4));
            BB_HIP(tmp.get(&pi, (size_t)nsplit * nq * 4));
            hipLaunchKernelGGL(k_assign_mfma, dim3((unsigned)qtiles, (unsigned)nsplit), dim3(256), 0, s, qd, nq, q_stride,
                               cd, (int)nc, per, qcard, ccard, pn, pu, pi);
        } else {
            const bool fast = al4 && (nbytes == 8 || nbytes == 16 || nbytes == 32 || nbytes == 64 || nbytes == 128 ||
                                      nbytes == 256);
            const int64_t qblocks = fast ? (nq + 255) / 256 : (nq + 3) / 4;
            int64_t want = (4 * (int64_t)cus + qblocks - 1) / qblocks;  // fill the device four times over
            const int64_t most = (nc + 63) / 64;                         // ... with at least 64 centroids per range
            if (want > most) want = most;
            if (want > 65535) want = 65535;
            const int per = (int)((nc + want - 1) / want);
            nsplit = (int)((nc + per - 1) / per);
            BB_HIP(tmp.get(&pn, (size_t)nsplit * nq * 4));
            BB_HIP(tmp.get(&pu, (size_t)nsplit * nq * 4));
            BB_HIP(tmp.get(&pi, (size_t)nsplit * nq * 4));
            const dim3 grid((unsigned)qblocks, (unsigned)nsplit);
#define BB_LAUNCH_ASSIGN(W)                                                                                   \
    hipLaunchKernelGGL((k_assign_bcnt<W>), grid, dim3(256), 0, s, qd, nq, q_stride, (const uint32_t*)cd, (int)nc, \
                       per, ccard, pn, pu, pi)
            if (!fast)
                hipLaunchKernelGGL(k_assign_generic, grid, dim3(256), 0, s, qd, nq, q_stride, cd, (int)nc, per, nbytes,
                                   ccard, pn, pu, pi);
            else if (nbytes == 8) BB_LAUNCH_ASSIGN(2);
            else if (nbytes == 16) BB_LAUNCH_ASSIGN(4);
            else if (nbytes == 32) BB_LAUNCH_ASSIGN(8);
            else if (nbytes == 64) BB_LAUNCH_ASSIGN(16);
            else if (nbytes == 128) BB_LAUNCH_ASSIGN(32);
            else BB_LAUNCH_ASSIGN(64);
#undef BB_LAUNCH_ASSIGN
        }
        BB_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_assign_combine, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, nq, nsplit, pn, pu, pi,
                           (int32_t*)oi.dev, (uint32_t*)on.dev, (uint32_t*)ou.dev);
        BB_HIP(hipGetLastError());
    }
    BB_TRY(oi.finish(s));
    BB_TRY(on.finish(s));
    BB_TRY(ou.finish(s));
    return tmp.sync();
}

extern "C" int bbh_jt_dist_matrix(const uint8_t* queries, int64_t nq, int64_t q_stride, const uint8_t* cents,
                                  int64_t nc, int64_t nbytes, double* out, void* stream) {
    BB_TRY(bb::ensure_device());
    if (nq < 0 || nc < 1 || nbytes <= 0 || q_stride < nbytes || out == nullptr)
        return bb::fail(BBH_ERR_INVALID, "dist_matrix: need nq >= 0, nc >= 1, q_stride >= nbytes and an output");
    if (nq == 0) return BBH_OK;
    hipStream_t s = (hipStream_t)stream;
    bb::DevIn q, c;
    bb::DevOut o;
    BB_TRY(q.init(queries, (size_t)((nq - 1) * q_stride + nbytes), s));
    BB_TRY(c.init(cents, (size_t)(nc * nbytes), s));
    BB_TRY(o.init(out, (size_t)nq * (size_t)nc * 8));
    const uint8_t* qd = (const uint8_t*)q.dev;
    const uint8_t* cd = (const uint8_t*)c.dev;
    const bool al4 = (uintptr_t)qd % 4 == 0 && (uintptr_t)cd % 4 == 0 && q_stride % 4 == 0;
    const bool fast = al4 && (nbytes == 8 || nbytes == 16 || nbytes == 32 || nbytes == 64 || nbytes == 128 ||
                              nbytes == 256);
    bb::DevScope tmp(s);
    {
        bb::ProfScope ps("jt_dist_matrix", s);
        ps.units(nq);
        const int64_t cblocks = (nc + 255) / 256;
        if (fast) {
            uint32_t* qcard = nullptr;
            BB_HIP(tmp.get(&qcard, (size_t)nq * 4));
            BB_TRY(bbh_popcount_rows(qd, nq, nbytes, q_stride, qcard, s));
            int64_t want = (4 * (int64_t)cu_count() + cblocks - 1) / cblocks;
            if (want > nq) want = nq;
            if (want > 65535) want = 65535;
            const int64_t per = (nq + want - 1) / want;
            const dim3 grid((unsigned)cblocks, (unsigned)((nq + per - 1) / per));
#define BB_LAUNCH_DIST(W)                                                                                          \
    hipLaunchKernelGGL((k_jaccard_dist<W>), grid, dim3(256), 0, s, qd, nq, q_stride, (const uint32_t*)cd, nc, per, \
                       qcard, (double*)o.dev)
            if (nbytes == 8) BB_LAUNCH_DIST(2);
            else if (nbytes == 16) BB_LAUNCH_DIST(4);
            else if (nbytes == 32) BB_LAUNCH_DIST(8);
            else if (nbytes == 64) BB_LAUNCH_DIST(16);
            else if (nbytes == 128) BB_LAUNCH_DIST(32);
            else BB_LAUNCH_DIST(64);
#undef BB_LAUNCH_DIST
        } else {
            const dim3 grid((unsigned)cblocks, (unsigned)(nq < 65535 ? nq : 65535), (unsigned)((nq + 65534) / 65535));
            hipLaunchKernelGGL(k_jaccard_dist_generic, grid, dim3(256), 0, s, qd, nq, q_stride, cd, nc, nbytes,
                               (double*)o.dev);
        }
        BB_HIP(hipGetLastError());
    }
    BB_TRY(o.finish(s));
    return tmp.sync();
}

// test hook of the operand-map probe: a (16 x 64 int8), b (64 x 16 int8), d (16 x 16 int32), host or device
extern "C" int bbh_mfma_i8_probe(const int8_t* a, const int8_t* b, int32_t* d, void* stream) {
    BB_TRY(bb::ensure_device());
    if (a == nullptr || b == nullptr || d == nullptr) return bb::fail(BBH_ERR_INVALID, "mfma probe: null pointer");
    hipStream_t s = (hipStream_t)stream;
    bb::DevIn da, db;
    bb::DevOut dd;
    BB_TRY(da.init(a, 16 * 64, s));
    BB_TRY(db.init(b, 64 * 16, s));
    BB_TRY(dd.init(d, 16 * 16 * 4));
    hipLaunchKernelGGL(k_mfma_i8_probe, dim3(1), dim3(64), 0, s, (const int8_t*)da.dev, (const int8_t*)db.dev,
                       (int32_t*)dd.dev);
    BB_HIP(hipGetLastError());
    BB_TRY(dd.finish(s));
    BB_HIP(hipStreamSynchronize(s));
    return BBH_OK;
}
