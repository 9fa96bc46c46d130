// bb_cluster_stats.hip -- what the clustering quality indices (bblean/metrics.py: jt_isim_chi :47, jt_dbi :108,
// jt_isim_dunn :163) need of every cluster, for all k clusters in one call, for gfx950 (MI355X, CDNA4).
//
//   bbh_cluster_stats_segments   majority-vote centroid, iSIM, distance of every member to the set's central, column sums
//     k_cs_small      sets of up to SMALL_MAX rows: one wave per set, everything in registers, no global intermediate
//     k_seg_colsum    larger sets: column counters of one set over many workgroups (bb_segments.h)
//     k_cs_finish     counters -> centroid words, S and Q, column sums
//     k_cs_dist       the row pass of a large set over the whole GPU (k_cs_dist_wide: rows of any width)
//   bbh_dbi_worst_ratios         the inner loop of the Davies-Bouldin index without a k x k array
//     k_dbi_popc, k_dbi_pairs
//
// Arithmetic.  The column counts of a set of m rows live in bit planes P_b (bit j of P_b = bit b of the count of column
// j), built by the ripple-carry add of bb_segments.h.  S = sum of the counts is the sum of the rows' popcounts and
// Q = sum of their squares = sum over plane pairs of 2^(b + c) popcount(P_b & P_c), as in bb_medoid.hip; the iSIM is
// isim_from_moments(S, Q, m) on these exact integers.  The centroid (centroid_from_sum: bit = 2 count >= m, for m = 1 the
// row itself) is count >= T with T = ceil(m / 2), and that comparison is made on all 32 columns of a word at once: walk
// the planes from the most significant one, keeping two masks, `gt` (columns already known to be above T) and `eq`
// (columns equal to T in every plane so far):   gt |= eq & P_b & ~T_b;   eq &= ~(P_b ^ T_b);   T_b is all ones or all
// zeros, T being the same for the whole wave.  The centroid word is gt | eq.  No column is ever extracted, except for
// out_sums.  The distance of a row x to the central c is 1.0 - i / max(double(|x| + |c| - i), 1.0) with i = |x & c|:
// bbh_jt_arr_vec's value and one subtraction, the reference's `1 - jt_sim_packed(clust, central)`.
//
// Which bit of a word is which column matters only to out_sums and to nothing else: ld_word puts byte o of a row into bits
// 8 (o % 4) .. 8 (o % 4) + 7 of word o / 4, and unpacking is MSB first, so bit t of word w is column
// (4 w + t / 8) * 8 + 7 - t % 8.
#include "bb_segments.h"

namespace {

constexpr long long NAN_BITS = 0x7ff8000000000000ll;

__device__ __forceinline__ int column_of(int w, int t) { return (4 * w + (t >> 3)) * 8 + 7 - (t & 7); }

// word `w` of a packed row of nb bytes, written bytewise where the row is not word-aligned or ends inside the word
__device__ __forceinline__ void st_word(uint8_t* row, int w, int nb, bool al, uint32_t v) {
    const int o = w * 4;
    if (o >= nb) return;
    if (al && o + 4 <= nb) {
        *reinterpret_cast<uint32_t*>(row + o) = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (o + k < nb) row[o + k] = (uint8_t)(v >> (8 * k));
}

// Distances of rows [i0, i1) of the set that starts at flat position `beg` to the central whose words are c (popcount
// pc), written in set order.  Rows of at most 512 bytes: a row's two counts are below 2^13 and share one reduction.
template <int WPL>
__device__ __forceinline__ void dist_pass(const Rows& R, const uint32_t (&c)[WPL], uint32_t pc, int64_t beg, int64_t i0,
                                          int64_t i1, int lane, double* __restrict__ out) {
    for (int64_t b0 = i0; b0 < i1; b0 += 64) {
        const int cnt = (int)(i1 - b0 < 64 ? i1 - b0 : 64);
        uint32_t mine = 0;
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
                uint32_t v = 0;
#pragma unroll
                for (int w = 0; w < WPL; ++w) v += ((uint32_t)__popc(x[j][w] & c[w]) << 16) + (uint32_t)__popc(x[j][w]);
                v = wave_total(v);
                if (lane == u0 + j) mine = v;
            }
        }
        if (lane < cnt) {
            const uint32_t inter = mine >> 16, card = mine & 0xffffu;
            out[beg + b0 + lane] = 1.0 - jt_from_counts(inter, card + pc - inter);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Sets of up to small_max rows, one wave per set (grid-stride over the sets).  Pass 1 adds the rows into the planes,
// the centroid word of every lane comes out of the planes, pass 2 measures the rows against it (or the given central).
// ---------------------------------------------------------------------------------------------------------------
template <int WPL>
__global__ __launch_bounds__(256) void k_cs_small(Rows R, const int64_t* __restrict__ offsets, int64_t k, int64_t small_max,
                                                  int nf, int n_words, bool need_planes, const uint8_t* __restrict__ centrals,
                                                  int64_t c_stride, bool c_al, uint8_t* __restrict__ out_cent, bool oc_al,
                                                  double* __restrict__ out_isim, double* __restrict__ out_dist,
                                                  unsigned long long* __restrict__ out_sums) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = uniform_i64((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t g = wave0; g < k; g += n_waves) {
        const int64_t beg = offsets[g];
        const int64_t m = offsets[g + 1] - beg;
        if (m > small_max) continue;  // the large path's
        uint32_t cw[WPL];
#pragma unroll
        for (int w = 0; w < WPL; ++w) cw[w] = 0;
        if (need_planes) {
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
            // count >= ceil(m / 2) on the 32 columns of a word at once, most significant plane first
            const uint32_t thr = (uint32_t)((m + 1) >> 1);
#pragma unroll
            for (int w = 0; w < WPL; ++w) {
                uint32_t gt = 0u, eq = ~0u;
#pragma unroll
                for (int b = SMALL_PLANES - 1; b >= 0; --b) {
                    const uint32_t tb = (thr >> b) & 1u ? ~0u : 0u;
                    gt |= eq & P[w][b] & ~tb;
                    eq &= ~(P[w][b] ^ tb);
                }
                cw[w] = gt | eq;
            }
            if (out_cent) {
#pragma unroll
                for (int w = 0; w < WPL; ++w) st_word(out_cent + g * R.nb, lane + 64 * w, R.nb, oc_al, cw[w]);
            }
            if (out_isim) {
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
                if (lane == 0)
                    out_isim[g] = m < 2 ? __longlong_as_double(NAN_BITS) : isim_from_moments(S, Q, (unsigned long long)m);
            }
            if (out_sums) {
#pragma unroll
                for (int w = 0; w < WPL; ++w) {
                    const int wi = lane + 64 * w;
                    if (wi < n_words) {
#pragma unroll
                        for (int t = 0; t < 32; ++t) {
                            uint32_t c = 0;
#pragma unroll
                            for (int b = 0; b < SMALL_PLANES; ++b) c |= ((P[w][b] >> t) & 1u) << b;
                            const int col = column_of(wi, t);
                            if (col < nf) out_sums[g * nf + col] = c;
                        }
                    }
                }
            }
        }
        if (out_dist) {
            if (centrals) {
#pragma unroll
                for (int w = 0; w < WPL; ++w) cw[w] = ld_word(centrals + g * c_stride, lane + 64 * w, R.nb, c_al);
            }
            uint32_t pcc = 0;
#pragma unroll
            for (int w = 0; w < WPL; ++w) pcc += __popc(cw[w]);
            dist_pass<WPL>(R, cw, wave_total(pcc), beg, 0, m, lane, out_dist);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Large path, one set per sequence of launches: k_seg_colsum, then one wave turns the counters into the set's centroid
// (as aligned words in cw, and as bytes in out_cent), its iSIM and its column sums.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cs_finish(const uint32_t* __restrict__ cnt, int n_words, int nb, int nf,
                                                  unsigned long long m, uint32_t* __restrict__ cw,
                                                  uint8_t* __restrict__ out_cent, double* __restrict__ out_isim,
                                                  unsigned long long* __restrict__ out_sums) {
    const int lane = threadIdx.x;
    unsigned long long s = 0, q = 0;
    for (int w = lane; w < n_words; w += 64) {
        uint32_t word = 0;
#pragma unroll 4
        for (int t = 0; t < 32; ++t) {
            const uint32_t c = cnt[(size_t)t * n_words + w];
            s += c;
            q += (unsigned long long)c * c;
            if (2ull * c >= m) word |= 1u << t;
            if (out_sums) {
                const int col = column_of(w, t);
                if (col < nf) out_sums[col] = c;
            }
        }
        cw[w] = word;
        if (out_cent) st_word(out_cent, w, nb, false, word);
    }
    s = wave_sum_u64(s);
    q = wave_sum_u64(q);
    if (lane == 0 && out_isim) *out_isim = m < 2 ? __longlong_as_double(NAN_BITS) : isim_from_moments(s, q, m);
}

// a wave measures a chunk of rows against the central held in registers
template <int WPL>
__global__ __launch_bounds__(256) void k_cs_dist(Rows R, int64_t beg, int64_t m, const uint8_t* __restrict__ central,
                                                 bool c_al, double* __restrict__ out_dist) {
    const int lane = threadIdx.x & 63;
    const int64_t i0 = uniform_i64(((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * CHUNK);
    if (i0 >= m) return;
    const int64_t i1 = i0 + CHUNK < m ? i0 + CHUNK : m;
    uint32_t cw[WPL];
    uint32_t pcc = 0;
#pragma unroll
    for (int w = 0; w < WPL; ++w) {
        cw[w] = ld_word(central, lane + 64 * w, R.nb, c_al);
        pcc += __popc(cw[w]);
    }
    dist_pass<WPL>(R, cw, wave_total(pcc), beg, i0, i1, lane, out_dist);
}

// rows of any width: a lane strides over the words, the central stays in memory (L1)
__global__ __launch_bounds__(256) void k_cs_dist_wide(Rows R, int64_t beg, int64_t m, int n_words,
                                                      const uint8_t* __restrict__ central, bool c_al,
                                                      double* __restrict__ out_dist) {
    const int lane = threadIdx.x & 63;
    const int64_t i0 = uniform_i64(((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * CHUNK);
    if (i0 >= m) return;
    const int64_t i1 = i0 + CHUNK < m ? i0 + CHUNK : m;
    uint32_t pcc = 0;
    for (int w = lane; w < n_words; w += 64) pcc += __popc(ld_word(central, w, R.nb, c_al));
    pcc = wave_total(pcc);
    for (int64_t b0 = i0; b0 < i1; b0 += 64) {
        const int cnt = (int)(i1 - b0 < 64 ? i1 - b0 : 64);
        uint32_t my_i = 0, my_p = 0;
        for (int u = 0; u < cnt; ++u) {
            const uint8_t* row = R.row(beg + b0 + u);
            uint32_t inter = 0, p = 0;
            for (int w = lane; w < n_words; w += 64) {
                const uint32_t x = ld_word(row, w, R.nb, R.al);
                inter += __popc(x & ld_word(central, w, R.nb, c_al));
                p += __popc(x);
            }
            inter = wave_total(inter);
            p = wave_total(p);
            if (lane == u) {
                my_i = inter;
                my_p = p;
            }
        }
        if (lane < cnt) out_dist[beg + b0 + lane] = 1.0 - jt_from_counts(my_i, my_p + pcc - my_i);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Davies-Bouldin: worst[i] = max over j != i of (scatter[i] + scatter[j]) / (1.0 - sim(i, j)).  A workgroup takes a
// tile of DBI_TILE centrals i against tiles of DBI_TILE centrals j, both in LDS DBI_WCH words at a time; a thread owns
// one i (its lane) and the DBI_TILE / 4 centrals j of its wave, whose words all lanes read as a broadcast.  The tiles
// j are dealt over gridDim.y workgroups; candidates are >= +0.0, +inf or a skipped NaN, so the parts merge with an
// integer maximum on the bit patterns.
// ---------------------------------------------------------------------------------------------------------------
constexpr int DBI_TILE = BBH_DBI_TILE;
constexpr int DBI_WCH = 64;
constexpr int DBI_LD = DBI_WCH + 1;  // odd leading dimension: the lanes' rows fall on different banks
constexpr int DBI_JPT = DBI_TILE / 4;
static_assert(DBI_TILE == 64, "a thread's i is its lane");

__global__ __launch_bounds__(256) void k_dbi_popc(const uint8_t* __restrict__ cents, int64_t k, int nb, int64_t stride,
                                                  bool al, int n_words, uint32_t* __restrict__ pc) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < k; i += (int64_t)gridDim.x * 256) {
        uint32_t p = 0;
        for (int w = 0; w < n_words; ++w) p += __popc(ld_word(cents + i * stride, w, nb, al));
        pc[i] = p;
    }
}

__global__ __launch_bounds__(256) void k_dbi_pairs(const uint8_t* __restrict__ cents, int64_t k, int nb, int64_t stride,
                                                   bool al, int n_words, const uint32_t* __restrict__ pc,
                                                   const double* __restrict__ scatter,
                                                   unsigned long long* __restrict__ worst, uint32_t* __restrict__ flags) {
    __shared__ uint32_t L[2 * DBI_TILE * DBI_LD];
    uint32_t* Li = L;
    uint32_t* Lj = L + DBI_TILE * DBI_LD;
    const int ti = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * DBI_TILE, i = i0 + ti;
    const bool i_ok = i < k;
    const double si = i_ok ? scatter[i] : 0.0;
    const uint32_t pi = i_ok ? pc[i] : 0u;
    const int64_t n_jt = (k + DBI_TILE - 1) / DBI_TILE;
    double best = 0.0;
    uint32_t f0 = 0, f1 = 0;
    for (int64_t jt = blockIdx.y; jt < n_jt; jt += gridDim.y) {
        const int64_t j0 = jt * DBI_TILE;
        uint32_t acc[DBI_JPT];
#pragma unroll
        for (int jj = 0; jj < DBI_JPT; ++jj) acc[jj] = 0;
        for (int wc = 0; wc < n_words; wc += DBI_WCH) {
            __syncthreads();  // the words of the turn before have been read
            for (int r = wv; r < DBI_TILE; r += 4) {
                const int64_t ri = i0 + r, rj = j0 + r;
                Li[r * DBI_LD + ti] = ri < k ? ld_word(cents + ri * stride, wc + ti, nb, al) : 0u;
                Lj[r * DBI_LD + ti] = rj < k ? ld_word(cents + rj * stride, wc + ti, nb, al) : 0u;
            }
            __syncthreads();
            const int nw = n_words - wc < DBI_WCH ? n_words - wc : DBI_WCH;
            for (int w = 0; w < nw; ++w) {
                const uint32_t xi = Li[ti * DBI_LD + w];
#pragma unroll
                for (int jj = 0; jj < DBI_JPT; ++jj) acc[jj] += __popc(xi & Lj[(wv * DBI_JPT + jj) * DBI_LD + w]);
            }
        }
#pragma unroll
        for (int jj = 0; jj < DBI_JPT; ++jj) {
            const int64_t j = j0 + wv * DBI_JPT + jj;
            if (i_ok && j < k && j != i) {
                const uint32_t inter = acc[jj];
                const double den = 1.0 - jt_from_counts(inter, pi + pc[j] - inter);
                const double num = si + scatter[j];
                const double cand = num / den;
                if (den == 0.0) {
                    if (num != 0.0) ++f0;
                    else ++f1;
                }
                if (cand > best) best = cand;  // (a NaN is never greater: skipped, like Python's max(max_d, x))
            }
        }
    }
    if (best > 0.0) atomicMax(&worst[i], (unsigned long long)__double_as_longlong(best));
    if (flags) {
        f0 = wave_total(f0);
        f1 = wave_total(f1);
        if (ti == 0) {
            if (f0) atomicAdd(&flags[0], f0);
            if (f1) atomicAdd(&flags[1], f1);
        }
    }
}

}  // namespace

extern "C" int bbh_cluster_stats_segments(const uint8_t* rows, int64_t n_rows, int64_t nbytes, int64_t row_stride,
                                          const int64_t* members, const int64_t* offsets, int64_t k, int64_t n_features,
                                          const uint8_t* centrals, int64_t centrals_stride, uint8_t* out_centroids,
                                          double* out_isim, double* out_dist, uint64_t* out_sums, void* stream) {
    static const char* const what = "cluster_stats_segments";
    BB_TRY(bb::ensure_device());
    hipStream_t s = (hipStream_t)stream;
    SegPlan plan;
    // (rows beyond the registers: every set takes the large path)
    BB_TRY(seg_plan_offsets(what, rows, n_rows, nbytes, row_stride, members, offsets, k, n_features, 0, s, plan));
    const int nb = (int)(n_features / 8);
    if (centrals != nullptr ? centrals_stride < nb : centrals_stride != 0)
        return bb::fail(BBH_ERR_INVALID, "%s: centrals need centrals_stride >= n_features / 8, and no centrals no stride", what);
    const int64_t* off = plan.off;
    const int n_words = plan.n_words;
    const int64_t total = plan.total;

    bb::DevIn d_rows, d_mem, d_off, d_cen;
    bb::DevOut o_cent, o_isim, o_dist, o_sums;
    bb::DevScope tmp(s);
    BB_TRY(d_mem.init(members, (size_t)total * 8, s));
    if (members != nullptr && bb::is_device_ptr(members)) BB_TRY(seg_check_members_dev(what, members, total, n_rows, s, tmp));
    BB_TRY(d_rows.init(rows, (size_t)((n_rows - 1) * row_stride + nbytes), s));
    BB_TRY(d_off.init(offsets, (size_t)(k + 1) * 8, s));
    BB_TRY(d_cen.init(centrals, centrals ? (size_t)((k - 1) * centrals_stride + nb) : 0, s));
    BB_TRY(o_cent.init(out_centroids, (size_t)k * nb));
    BB_TRY(o_isim.init(out_isim, (size_t)k * 8));
    BB_TRY(o_dist.init(out_dist, (size_t)total * 8));
    BB_TRY(o_sums.init(out_sums, (size_t)k * (size_t)n_features * 8));

    Rows R;
    R.base = (const uint8_t*)d_rows.dev;
    R.stride = row_stride;
    R.members = (const int64_t*)d_mem.dev;
    R.nb = nb;
    R.al = (uintptr_t)R.base % 4 == 0 && row_stride % 4 == 0;
    const uint8_t* cen = (const uint8_t*)d_cen.dev;
    const bool c_al = (uintptr_t)cen % 4 == 0 && centrals_stride % 4 == 0;
    uint8_t* oc = (uint8_t*)o_cent.dev;
    const bool oc_al = (uintptr_t)oc % 4 == 0 && nb % 4 == 0;
    double* oi = (double*)o_isim.dev;
    double* od = (double*)o_dist.dev;
    unsigned long long* os = (unsigned long long*)o_sums.dev;
    // the planes / counters are needed for everything but distances to given centrals
    const bool need_planes = oc != nullptr || oi != nullptr || os != nullptr || (od != nullptr && cen == nullptr);

    if (need_planes || od != nullptr) {
        if (plan.n_small > 0) {
            bb::ProfScope ps("cluster_stats_seg/small", s);
            ps.units(plan.small_rows);
            int64_t waves = (int64_t)seg_cu_count() * 32;
            if (waves > k) waves = k;
            const dim3 grid((unsigned)((waves + 3) / 4));
            if (n_words <= 64)
                hipLaunchKernelGGL((k_cs_small<1>), grid, dim3(256), 0, s, R, (const int64_t*)d_off.dev, k, plan.small_max,
                                   (int)n_features, n_words, need_planes, cen, centrals_stride, c_al, oc, oc_al, oi, od, os);
            else
                hipLaunchKernelGGL((k_cs_small<2>), grid, dim3(256), 0, s, R, (const int64_t*)d_off.dev, k, plan.small_max,
                                   (int)n_features, n_words, need_planes, cen, centrals_stride, c_al, oc, oc_al, oi, od, os);
            BB_HIP(hipGetLastError());
        }
        if (plan.n_large > 0) {
            bb::ProfScope ps("cluster_stats_seg/large", s);
            ps.units(plan.large_rows);
            uint32_t *cnt = nullptr, *cw = nullptr;
            BB_HIP(tmp.get(&cnt, (size_t)n_words * 32 * 4));
            BB_HIP(tmp.get(&cw, (size_t)n_words * 4));
            for (int64_t g = 0; g < k; ++g) {
                const int64_t beg = off[g], m = off[g + 1] - beg;
                if (m <= plan.small_max) continue;
                const int64_t chunks = (m + CHUNK - 1) / CHUNK;
                const dim3 grid((unsigned)((chunks + 3) / 4));
                if (need_planes) {
                    BB_HIP(hipMemsetAsync(cnt, 0, (size_t)n_words * 32 * 4, s));
                    hipLaunchKernelGGL(k_seg_colsum, grid, dim3(256), 0, s, R, beg, m, n_words, cnt);
                    hipLaunchKernelGGL(k_cs_finish, dim3(1), dim3(64), 0, s, cnt, n_words, nb, (int)n_features,
                                       (unsigned long long)m, cw, oc ? oc + g * nb : nullptr, oi ? oi + g : nullptr,
                                       os ? os + g * n_features : nullptr);
                }
                if (od != nullptr) {
                    const uint8_t* central = cen ? cen + g * centrals_stride : (const uint8_t*)cw;
                    const bool al = cen ? c_al : true;
                    if (!plan.regs)
                        hipLaunchKernelGGL(k_cs_dist_wide, grid, dim3(256), 0, s, R, beg, m, n_words, central, al, od);
                    else if (n_words <= 64)
                        hipLaunchKernelGGL((k_cs_dist<1>), grid, dim3(256), 0, s, R, beg, m, central, al, od);
                    else
                        hipLaunchKernelGGL((k_cs_dist<2>), grid, dim3(256), 0, s, R, beg, m, central, al, od);
                }
                BB_HIP(hipGetLastError());
            }
        }
    }
    BB_TRY(o_cent.finish(s));
    BB_TRY(o_isim.finish(s));
    BB_TRY(o_dist.finish(s));
    BB_TRY(o_sums.finish(s));
    return tmp.sync();
}

extern "C" int bbh_dbi_worst_ratios(const uint8_t* centrals, int64_t k, int64_t nbytes, int64_t stride,
                                    const double* scatter, double* out_worst, uint32_t* out_flags, void* stream) {
    BB_TRY(bb::ensure_device());
    if (centrals == nullptr || scatter == nullptr || out_worst == nullptr || k < 1 || nbytes <= 0 || stride < nbytes ||
        nbytes > 0x7fffffffll / 8)
        return bb::fail(BBH_ERR_INVALID, "dbi_worst_ratios: need centrals, scatter, out_worst, k >= 1 and stride >= nbytes");
    hipStream_t s = (hipStream_t)stream;
    bb::DevIn d_cen, d_sc;
    bb::DevOut o_worst, o_flags;
    bb::DevScope tmp(s);
    BB_TRY(d_cen.init(centrals, (size_t)((k - 1) * stride + nbytes), s));
    BB_TRY(d_sc.init(scatter, (size_t)k * 8, s));
    BB_TRY(o_worst.init(out_worst, (size_t)k * 8));
    BB_TRY(o_flags.init(out_flags, 8));
    const uint8_t* cen = (const uint8_t*)d_cen.dev;
    const bool al = (uintptr_t)cen % 4 == 0 && stride % 4 == 0;
    const int n_words = (int)((nbytes + 3) / 4);
    BB_HIP(hipMemsetAsync(o_worst.dev, 0, (size_t)k * 8, s));  // +0.0, where the maximum starts
    if (o_flags.dev) BB_HIP(hipMemsetAsync(o_flags.dev, 0, 8, s));
    if (k > 1) {
        bb::ProfScope ps("dbi_pairs", s);
        ps.units((long long)k * (long long)(k - 1));
        uint32_t* pc = nullptr;
        BB_HIP(tmp.get(&pc, (size_t)k * 4));
        int64_t blocks = (k + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(k_dbi_popc, dim3((unsigned)blocks), dim3(256), 0, s, cen, k, (int)nbytes, stride, al, n_words, pc);
        const int64_t n_tiles = (k + DBI_TILE - 1) / DBI_TILE;
        int64_t parts = ((int64_t)seg_cu_count() * 4 + n_tiles - 1) / n_tiles;  // enough workgroups to fill the GPU
        if (parts > n_tiles) parts = n_tiles;
        if (parts > 65535) parts = 65535;
        hipLaunchKernelGGL(k_dbi_pairs, dim3((unsigned)n_tiles, (unsigned)parts), dim3(256), 0, s, cen, k, (int)nbytes, stride,
                           al, n_words, (const uint32_t*)pc, (const double*)d_sc.dev, (unsigned long long*)o_worst.dev,
                           (uint32_t*)o_flags.dev);
        BB_HIP(hipGetLastError());
    }
    BB_TRY(o_worst.finish(s));
    BB_TRY(o_flags.finish(s));
    return tmp.sync();
}
