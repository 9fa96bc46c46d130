// bb_medoid.hip -- segmented complementary iSIM (jt_compl_isim / jt_isim_medoid of the reference,
// bblean/_py_similarity.py:65-117) of k independent sets of packed rows in one call, for gfx950 (MI355X, CDNA4).
//
//   bbh_compl_isim_segments
//     k_seg_small     sets of up to SMALL_MAX rows: one wave per set, everything in registers, no global intermediate
//     k_seg_colsum    larger sets: column counters of one set over many workgroups (uint32 atomics)
//     k_seg_planes    counters -> bit planes, S and Q
//     k_seg_rows      the row pass over the whole GPU, one (value, position) winner per wave
//     k_seg_argmin    the winners of the waves -> the set's medoid position
//     k_seg_check     index check of a device-resident `members`
//
// Arithmetic.  For a set of m >= 3 rows x_r with column sums ls_j, S = sum ls_j and Q = sum ls_j^2, the reference
// evaluates jt_isim_from_sum(ls - x_r, m - 1) for every row.  The rows are 0/1, so with
//        p_r = popcount(x_r),   d_r = sum of ls_j over the set bits j of x_r
// the moments of ls - x_r are s_r = S - p_r and q_r = Q - 2 d_r + p_r: exact integers, then isim_from_moments as it is.
// d_r needs no unpacking: with ls written as bit planes P_b (bit j of P_b = bit b of ls_j),
//        d_r = sum_b 2^b popcount(x_r & P_b).
// The planes themselves come from a bit-sliced counter: adding a row x to the planes is a ripple-carry add over whole
// words (carry = x; t = P_b & carry; P_b ^= carry; carry = t), two VALU operations per plane and 32 columns - no
// per-column counter, no LDS, no bank conflict.  A lane owns word `lane` (and `lane + 64` for rows of more than 256
// bytes) of every row and of every plane; which bit of a word is which column never matters, rows and planes share it.
//
// Values are >= +0.0 and never NaN (isim_from_moments: q - s >= 0 and the denominator is >= the numerator), so
// their bit patterns order like the values and the first minimum is an integer reduction on (bits, position).
#include "bb_segments.h"

#include <cmath>

using namespace bbd;

namespace {

constexpr int GRP = 12;         // planes per uint32 partial of d_r: 64 columns per lane * 2^12 * 64 lanes = 2^24
constexpr unsigned long long NO_KEY = ~0ull;

// Pass over rows [i0, i1) of the set that starts at flat position `beg`: value of every row, written to out (set
// order) when asked for; every lane keeps the first minimum among the rows it evaluated (rows i with i % 64 == lane).
template <int WPL, int NP>
__device__ __forceinline__ void compl_pass(const Rows& R, const uint32_t (&P)[WPL][NP], unsigned long long S,
                                           unsigned long long Q, unsigned long long m, int64_t beg, int64_t i0, int64_t i1,
                                           int lane, double* __restrict__ out, unsigned long long& best_key,
                                           int64_t& best_pos) {
    constexpr int NG = (NP + GRP - 1) / GRP;
    for (int64_t b0 = i0; b0 < i1; b0 += 64) {
        const int cnt = (int)(i1 - b0 < 64 ? i1 - b0 : 64);
        uint32_t my_p = 0;
        unsigned long long my_d = 0;
        for (int u0 = 0; u0 < cnt; u0 += 4) {
            uint32_t x[4][WPL];
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // (rows behind the last are the last again: loaded, evaluated, not kept)
                const int u = u0 + j < cnt ? u0 + j : cnt - 1;
                const uint8_t* row = R.row(beg + b0 + u);
#pragma unroll
                for (int w = 0; w < WPL; ++w) x[j][w] = ld_word(row, lane + 64 * w, R.nb, R.al);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t p = 0, g[NG];
#pragma unroll
                for (int q = 0; q < NG; ++q) g[q] = 0;
#pragma unroll
                for (int w = 0; w < WPL; ++w) {
                    p += __popc(x[j][w]);
#pragma unroll
                    for (int b = 0; b < NP; ++b) g[b / GRP] += (uint32_t)__popc(x[j][w] & P[w][b]) << (b % GRP);
                }
                p = wave_total(p);
                unsigned long long d = 0;
#pragma unroll
                for (int q = 0; q < NG; ++q) d += (unsigned long long)wave_total(g[q]) << (GRP * q);
                if (lane == u0 + j) {
                    my_p = p;
                    my_d = d;
                }
            }
        }
        if (lane < cnt) {
            const double v = isim_from_moments(S - my_p, Q - 2ull * my_d + my_p, m - 1ull);
            if (out) out[beg + b0 + lane] = v;
            const unsigned long long key = (unsigned long long)__double_as_longlong(v);
            if (key < best_key) {  // strict: an earlier row of this lane stays
                best_key = key;
                best_pos = b0 + lane;
            }
        }
    }
}

// (key, position) of the lanes -> the wave's first minimum, in every lane
__device__ __forceinline__ void wave_first_min(unsigned long long& key, int64_t& pos) {
    const unsigned long long kmin = wave_min_u64(key);
    const unsigned long long cand = key == kmin ? (unsigned long long)pos : NO_KEY;
    key = kmin;
    pos = (int64_t)wave_min_u64(cand);
}

// ---------------------------------------------------------------------------------------------------------------
// Sets of up to small_max rows, one wave per set (grid-stride over the sets, so the one- and two-row majority costs
// two scalar loads and a store each).  Pass 1 adds the rows into the planes, pass 2 evaluates them.
// ---------------------------------------------------------------------------------------------------------------
template <int WPL>
__global__ __launch_bounds__(256) void k_seg_small(Rows R, const int64_t* __restrict__ offsets, int64_t k,
                                                   int64_t small_max, double* __restrict__ out_compl,
                                                   int64_t* __restrict__ out_medoid) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = uniform_i64((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t g = wave0; g < k; g += n_waves) {
        const int64_t beg = offsets[g];
        const int64_t m = offsets[g + 1] - beg;
        if (m < 3) {  // _py_similarity.py:74-77, :110-111
            if (out_compl && lane < m) out_compl[beg + lane] = __longlong_as_double(0x7ff8000000000000ll);
            if (out_medoid && lane == 0) out_medoid[g] = 0;
            continue;
        }
        if (m > small_max) continue;  // the large path's
        uint32_t P[WPL][SMALL_PLANES];
#pragma unroll
        for (int w = 0; w < WPL; ++w)
#pragma unroll
            for (int b = 0; b < SMALL_PLANES; ++b) P[w][b] = 0;
        uint32_t pc = 0;
        for (int64_t i = 0; i < m; i += 4) {
            uint32_t x[4][WPL];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = i + j < m;
                const uint8_t* row = R.row(beg + (ok ? i + j : m - 1));
#pragma unroll
                for (int w = 0; w < WPL; ++w) {
                    const uint32_t v = ld_word(row, lane + 64 * w, R.nb, R.al);
                    x[j][w] = ok ? v : 0u;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int w = 0; w < WPL; ++w) pc += __popc(x[j][w]);
                planes_add<WPL, SMALL_PLANES>(P, x[j]);
            }
        }
        // S = sum of the counts, Q = sum of their squares = sum over plane pairs of 2^(b + c) popcount(P_b & P_c)
        unsigned long long q = 0;
#pragma unroll
        for (int b = 0; b < SMALL_PLANES; ++b)
#pragma unroll
            for (int c = b; c < SMALL_PLANES; ++c) {
                uint32_t n = 0;
#pragma unroll
                for (int w = 0; w < WPL; ++w) n += __popc(P[w][b] & P[w][c]);
                q += (unsigned long long)n << (b + c + (b != c ? 1 : 0));
            }
        const unsigned long long S = wave_sum_u64((unsigned long long)pc);
        const unsigned long long Q = wave_sum_u64(q);
        unsigned long long key = NO_KEY;
        int64_t pos = 0;
        compl_pass<WPL, SMALL_PLANES>(R, P, S, Q, (unsigned long long)m, beg, 0, m, lane, out_compl, key, pos);
        if (out_medoid) {
            wave_first_min(key, pos);
            if (lane == 0) out_medoid[g] = pos;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Large path, one set per sequence of launches (k_seg_colsum and its counters: bb_segments.h).
// ---------------------------------------------------------------------------------------------------------------
// one wave: counters -> planes[b * n_words + w] (32 planes), hdr[0] = S, hdr[1] = Q
__global__ __launch_bounds__(64) void k_seg_planes(const uint32_t* __restrict__ cnt, int n_words,
                                                   uint32_t* __restrict__ planes, unsigned long long* __restrict__ hdr) {
    const int lane = threadIdx.x;
    unsigned long long s = 0, q = 0;
    for (int w = lane; w < n_words; w += 64) {
        uint32_t P[32];
#pragma unroll
        for (int b = 0; b < 32; ++b) P[b] = 0;
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const uint32_t c = cnt[(size_t)t * n_words + w];
            s += c;
            q += (unsigned long long)c * c;
#pragma unroll
            for (int b = 0; b < 32; ++b) P[b] |= ((c >> b) & 1u) << t;
        }
#pragma unroll
        for (int b = 0; b < 32; ++b) planes[(size_t)b * n_words + w] = P[b];
    }
    s = wave_sum_u64(s);
    q = wave_sum_u64(q);
    if (lane == 0) {
        hdr[0] = s;
        hdr[1] = q;
    }
}

// a wave evaluates a chunk of rows against planes held in registers; one winner per wave
template <int WPL, int NP>
__global__ __launch_bounds__(256) void k_seg_rows(Rows R, int64_t beg, int64_t m, int n_words,
                                                  const uint32_t* __restrict__ planes,
                                                  const unsigned long long* __restrict__ hdr, double* __restrict__ out_compl,
                                                  unsigned long long* __restrict__ part_key, int64_t* __restrict__ part_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t chunk = uniform_i64((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    const int64_t i0 = chunk * CHUNK;
    if (i0 >= m) return;
    const int64_t i1 = i0 + CHUNK < m ? i0 + CHUNK : m;
    uint32_t P[WPL][NP];
#pragma unroll
    for (int w = 0; w < WPL; ++w)
#pragma unroll
        for (int b = 0; b < NP; ++b) P[w][b] = lane + 64 * w < n_words ? planes[(size_t)b * n_words + lane + 64 * w] : 0u;
    unsigned long long key = NO_KEY;
    int64_t pos = 0;
    compl_pass<WPL, NP>(R, P, hdr[0], hdr[1], (unsigned long long)m, beg, i0, i1, lane, out_compl, key, pos);
    if (part_key) {
        wave_first_min(key, pos);
        if (lane == 0) {
            part_key[chunk] = key;
            part_pos[chunk] = pos;
        }
    }
}

// rows of any width: the planes stay in memory (L2), a lane strides over the words
__global__ __launch_bounds__(256) void k_seg_rows_wide(Rows R, int64_t beg, int64_t m, int n_words, int n_planes,
                                                       const uint32_t* __restrict__ planes,
                                                       const unsigned long long* __restrict__ hdr,
                                                       double* __restrict__ out_compl, unsigned long long* __restrict__ part_key,
                                                       int64_t* __restrict__ part_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t chunk = uniform_i64((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    const int64_t i0 = chunk * CHUNK;
    if (i0 >= m) return;
    const int64_t i1 = i0 + CHUNK < m ? i0 + CHUNK : m;
    const unsigned long long S = hdr[0], Q = hdr[1];
    unsigned long long key = NO_KEY;
    int64_t pos = 0;
    for (int64_t b0 = i0; b0 < i1; b0 += 64) {
        const int cnt = (int)(i1 - b0 < 64 ? i1 - b0 : 64);
        uint32_t my_p = 0;
        unsigned long long my_d = 0;
        for (int u = 0; u < cnt; ++u) {
            const uint8_t* row = R.row(beg + b0 + u);
            uint32_t p = 0;
            unsigned long long d = 0;
            for (int w = lane; w < n_words; w += 64) {
                const uint32_t x = ld_word(row, w, R.nb, R.al);
                p += __popc(x);
                for (int b = 0; b < n_planes; ++b)
                    d += (unsigned long long)__popc(x & planes[(size_t)b * n_words + w]) << b;
            }
            p = (uint32_t)wave_sum_u64(p);
            d = wave_sum_u64(d);
            if (lane == u) {
                my_p = p;
                my_d = d;
            }
        }
        if (lane < cnt) {
            const double v = isim_from_moments(S - my_p, Q - 2ull * my_d + my_p, (unsigned long long)m - 1ull);
            if (out_compl) out_compl[beg + b0 + lane] = v;
            const unsigned long long kk = (unsigned long long)__double_as_longlong(v);
            if (kk < key) {
                key = kk;
                pos = b0 + lane;
            }
        }
    }
    if (part_key) {
        wave_first_min(key, pos);
        if (lane == 0) {
            part_key[chunk] = key;
            part_pos[chunk] = pos;
        }
    }
}

// one workgroup: the first minimum over the waves' winners
__global__ __launch_bounds__(256) void k_seg_argmin(const unsigned long long* __restrict__ part_key,
                                                    const int64_t* __restrict__ part_pos, int64_t n,
                                                    int64_t* __restrict__ out) {
    __shared__ unsigned long long sk[4];
    __shared__ int64_t sp[4];
    unsigned long long key = NO_KEY;
    int64_t pos = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const unsigned long long kk = part_key[i];
        const int64_t pp = part_pos[i];
        if (kk < key || (kk == key && pp < pos)) {
            key = kk;
            pos = pp;
        }
    }
    wave_first_min(key, pos);
    if ((threadIdx.x & 63) == 0) {
        sk[threadIdx.x >> 6] = key;
        sp[threadIdx.x >> 6] = pos;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (sk[w] < key || (sk[w] == key && sp[w] < pos)) {
                key = sk[w];
                pos = sp[w];
            }
        *out = pos;
    }
}

}  // namespace

extern "C" int bbh_compl_isim_segments(const uint8_t* rows, int64_t n_rows, int64_t nbytes, int64_t row_stride,
                                       const int64_t* members, const int64_t* offsets, int64_t k, int64_t n_features,
                                       double* out_compl, int64_t* out_medoid, void* stream) {
    BB_TRY(bb::ensure_device());
    hipStream_t s = (hipStream_t)stream;
    SegPlan plan;
    BB_TRY(seg_plan_offsets("compl_isim_segments", rows, n_rows, nbytes, row_stride, members, offsets, k, n_features, 2, s,
                            plan));
    const int64_t* off = plan.off;
    const int n_words = plan.n_words;
    const bool regs = plan.regs;
    const int64_t small_max = plan.small_max, small_rows = plan.small_rows, n_small = plan.n_small,
                  large_rows = plan.large_rows, n_large = plan.n_large, largest = plan.largest, total = plan.total;

    bb::DevIn d_rows, d_mem, d_off;
    bb::DevOut o_compl, o_med;
    bb::DevScope tmp(s);
    BB_TRY(d_mem.init(members, (size_t)total * 8, s));
    if (members != nullptr && bb::is_device_ptr(members))
        BB_TRY(seg_check_members_dev("compl_isim_segments", members, total, n_rows, s, tmp));
    BB_TRY(d_rows.init(rows, (size_t)((n_rows - 1) * row_stride + nbytes), s));
    BB_TRY(d_off.init(offsets, (size_t)(k + 1) * 8, s));
    BB_TRY(o_compl.init(out_compl, (size_t)total * 8));
    BB_TRY(o_med.init(out_medoid, (size_t)k * 8));

    Rows R;
    R.base = (const uint8_t*)d_rows.dev;
    R.stride = row_stride;
    R.members = (const int64_t*)d_mem.dev;
    R.nb = (int)(n_features / 8);
    R.al = (uintptr_t)R.base % 4 == 0 && row_stride % 4 == 0;
    double* oc = (double*)o_compl.dev;
    int64_t* om = (int64_t*)o_med.dev;

    if (oc != nullptr || om != nullptr) {
        if (n_small > 0) {  // every set of up to small_max rows, the one- and two-row sets among them
            bb::ProfScope ps("compl_isim_seg/small", s);
            ps.units(small_rows);
            int64_t waves = (int64_t)seg_cu_count() * 32;
            if (waves > k) waves = k;
            const dim3 grid((unsigned)((waves + 3) / 4));
            if (n_words <= 64)
                hipLaunchKernelGGL((k_seg_small<1>), grid, dim3(256), 0, s, R, (const int64_t*)d_off.dev, k, small_max, oc, om);
            else
                hipLaunchKernelGGL((k_seg_small<2>), grid, dim3(256), 0, s, R, (const int64_t*)d_off.dev, k, small_max, oc, om);
            BB_HIP(hipGetLastError());
        }
        if (n_large > 0) {
            bb::ProfScope ps("compl_isim_seg/large", s);
            ps.units(large_rows);
            const int64_t max_chunks = (largest + CHUNK - 1) / CHUNK;
            uint32_t *cnt = nullptr, *planes = nullptr;
            unsigned long long *hdr = nullptr, *pk = nullptr;
            int64_t* pp = nullptr;
            BB_HIP(tmp.get(&cnt, (size_t)n_words * 32 * 4));
            BB_HIP(tmp.get(&planes, (size_t)n_words * 32 * 4));
            BB_HIP(tmp.get(&hdr, 16));
            if (om) {
                BB_HIP(tmp.get(&pk, (size_t)max_chunks * 8));
                BB_HIP(tmp.get(&pp, (size_t)max_chunks * 8));
            }
            for (int64_t g = 0; g < k; ++g) {
                const int64_t beg = off[g], m = off[g + 1] - beg;
                if (m <= small_max) continue;
                const int64_t chunks = (m + CHUNK - 1) / CHUNK;
                const dim3 grid((unsigned)((chunks + 3) / 4));
                const int np = bit_length(m);
                BB_HIP(hipMemsetAsync(cnt, 0, (size_t)n_words * 32 * 4, s));
                hipLaunchKernelGGL(k_seg_colsum, grid, dim3(256), 0, s, R, beg, m, n_words, cnt);
                hipLaunchKernelGGL(k_seg_planes, dim3(1), dim3(64), 0, s, cnt, n_words, planes, hdr);
#define BB_LAUNCH_ROWS(W, NP) \
    hipLaunchKernelGGL((k_seg_rows<W, NP>), grid, dim3(256), 0, s, R, beg, m, n_words, planes, hdr, oc, pk, pp)
                if (!regs)
                    hipLaunchKernelGGL(k_seg_rows_wide, grid, dim3(256), 0, s, R, beg, m, n_words, np, planes, hdr, oc, pk, pp);
                else if (n_words <= 64) {
                    if (np <= 16) BB_LAUNCH_ROWS(1, 16);
                    else if (np <= 20) BB_LAUNCH_ROWS(1, 20);
                    else if (np <= 24) BB_LAUNCH_ROWS(1, 24);
                    else BB_LAUNCH_ROWS(1, 32);
                } else {
                    if (np <= 16) BB_LAUNCH_ROWS(2, 16);
                    else if (np <= 20) BB_LAUNCH_ROWS(2, 20);
                    else if (np <= 24) BB_LAUNCH_ROWS(2, 24);
                    else BB_LAUNCH_ROWS(2, 32);
                }
#undef BB_LAUNCH_ROWS
                if (om) hipLaunchKernelGGL(k_seg_argmin, dim3(1), dim3(256), 0, s, pk, pp, chunks, om + g);
                BB_HIP(hipGetLastError());
            }
        }
    }
    BB_TRY(o_compl.finish(s));
    BB_TRY(o_med.finish(s));
    return tmp.sync();
}
