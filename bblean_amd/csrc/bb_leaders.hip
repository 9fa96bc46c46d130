// bb_leaders.hip -- leader clustering (sphere exclusion, Taylor-Butina) of a packed table at a Jaccard distance, for gfx950
// (MI355X, CDNA4): the second consumer of bb_radius.hip's graph that never stores an edge.  DESIGN.md section 5i.
//
//   bbh_jt_leaders       centre, label (rank of the centre), number of clusters and density of every row
//     k_radius_table     imin[u], the smallest passing intersection of every union (bb_radius_common.h)
//     k_ld_init          density = weight, no neighbour seen, every row its own centre
//     k_ld_pairs         AND + popcount, lane per row, for the usual widths (k_cc_pairs' counting loop); one body, four uses:
//                          degree  the original table against itself, upper triangle: a hit adds to both densities
//                          cover   undecided rows against the centres of the round before: a hit makes a member
//                          block   undecided rows against undecided rows at a smaller position: a hit blocks
//                          assign  members against all centres: the smallest position among the hits
//     k_ld_pairs_generic every other width and alignment: one wave per row, the float64 division itself
//     k_ld_gather        the rows that have a neighbour, in priority order, zero-padded to an instantiated width
//     k_ld_round_scan    one workgroup: unblocked rows become centres, the undecided rows stay compacted in order
//     k_ld_step          the tail: one launch per remaining position, a centre takes its later undecided neighbours
//     k_ld_final_scan    one workgroup: the centres and the members, each compacted in priority order
//     k_ld_scatter       centre[original row]
//     k_ld_rank / k_ld_label   label[v] = rank of v's centre among the centres in ascending row index
//
// Rows a != b are neighbours iff bbh_jt_radius reports the pair: jaccard_dist(i, u) <= radius in float64.  density[a] =
// w[a] + the weights of a's neighbours.  Priority: higher density first, then the lower row (BBH_LEADERS_TIES_HIGH: the
// higher row).  The centres are the lexicographically first maximal independent set under that order and every other row
// belongs to its highest-priority neighbouring centre, which is what walking the rows in priority order gives.
//
// The one rule of the design: nothing in a kernel depends on what another workgroup stores in the same launch.  Every
// dependency crosses a kernel boundary; inside a launch workgroups only meet in commutative atomics (atomicAdd, atomicOr,
// atomicMin) whose results a later launch reads.  No thread waits on another; no flags, no fences, no inline assembly.  So
// the result is a function of rows, radius, weights and flag alone: not of the kernel that served a width, the grid, the
// order of the workgroups or the number of rounds that ran before the tail.
#include <algorithm>
#include <cstdlib>

#include "bb_common.h"
#include "bb_radius_common.h"  // jaccard_dist, k_radius_table, radius_ranges, radius_fast_width

using namespace bbd;

namespace {

constexpr int LD_FILL = 64;        // bb_components.hip's CC_FILL: triangles want many more blocks than slots
constexpr int LD_ROUND_CAP = 64;   // rounds before the tail at the latest
constexpr int64_t LD_SLOW = 64;    // the tail starts when two rounds decided less than 1 / LD_SLOW of their rows
constexpr int LD_NONE = 0x7fffffff;

enum : int { ST_UNDECIDED = 0, ST_CENTRE = 1, ST_MEMBER = 2 };
enum : int { LD_DEGREE = 0, LD_COVER = 1, LD_BLOCK = 2, LD_ASSIGN = 3 };

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void k_ld_init(int n, const uint32_t* __restrict__ w, u64* __restrict__ dens,
                                                 int* __restrict__ mark, int32_t* __restrict__ centre) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    dens[v] = w != nullptr ? (u64)w[v] : 1ull;
    mark[v] = 0;
    centre[v] = (int32_t)v;
}

// radius >= 1: one workgroup sums the weights
__global__ __launch_bounds__(1024) void k_ld_total(int n, const uint32_t* __restrict__ w, u64* __restrict__ total) {
    __shared__ u64 part[16];
    const int tid = (int)threadIdx.x;
    u64 s = 0;
    for (int64_t i = tid; i < n; i += 1024) s += w != nullptr ? (u64)w[i] : 1ull;
    s = wave_sum_u64(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        u64 t = 0;
        for (int k = 0; k < 16; ++k) t += part[k];
        *total = t;
    }
}

__global__ __launch_bounds__(256) void k_ld_fill_all(int n, const u64* __restrict__ total, int lead,
                                                     u64* __restrict__ dens, int32_t* __restrict__ centre) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    dens[v] = *total;
    centre[v] = lead;
}

// ---------------------------------------------------------------------------------------------------------------
// The pair loop.  A lane owns row qlist[jq] (degree: row jq) in registers and meets the rows mlist[m] (degree: row m) of
// its range; table rows are wave-uniform (scalar loads), imin[u] sits in LDS.  Grid: x = tiles of 256 lanes, y = ranges
// of the table side.  What a hit does is kept in registers and leaves the lane once, after the loop, as one atomic.
//   degree  m > jq.  sum += w[m]; density[m] += w[jq]; both rows have a neighbour.  `aux` = the marks.
//   cover   the lanes are undecided (the list holds nothing else).  A hit: state |= member.
//   block   lanes and table share one list; m < jq, both still undecided after the cover pass, which ran in an earlier
//           launch.  A hit: aux[row] |= 1 (blocked).  The state is only read.
//   assign  aux[row] = min(aux[row], m): the smallest position in the list of centres.
// ---------------------------------------------------------------------------------------------------------------
template <int W32, int MODE>
__global__ __launch_bounds__(256) void k_ld_pairs(const uint32_t* __restrict__ c, const uint32_t* __restrict__ card,
                                                  const uint16_t* __restrict__ tab, const int* __restrict__ qlist, int nq,
                                                  const int* __restrict__ mlist, int nm, int per,
                                                  const uint32_t* __restrict__ w, u64* dens, int* aux, int* state) {
    __shared__ uint16_t imin[W32 * 32 + 2];
    const int tid = (int)threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * 256;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    int m1 = (int)min((int64_t)nm, r0 + per);
    if (MODE == LD_DEGREE && (int64_t)m1 - 1 <= q0) return;  // the whole range lies at or below the tile
    if (MODE == LD_BLOCK && r0 >= q0 + 255) return;          // the whole range lies at or above the tile
    for (int u = tid; u <= W32 * 32; u += 256) imin[u] = tab[u];
    const int64_t jq = q0 + tid;
    const bool ok = jq < nq;
    const int row = ok ? (MODE == LD_DEGREE ? (int)jq : qlist[jq]) : 0;
    bool live = ok;
    if (MODE == LD_BLOCK) live = ok && state[row] == ST_UNDECIDED;
    const uint32_t* src = c + (size_t)row * W32;
    uint32_t x[W32];
    uint32_t qc = 0;
#pragma unroll
    for (int k = 0; k < W32; ++k) {
        x[k] = live ? src[k] : 0u;
        qc += __popc(x[k]);
    }
    __syncthreads();
    int m0 = (int)r0;
    if (MODE == LD_DEGREE) m0 = (int)min((int64_t)m1, max(r0, q0 + (tid & ~63) + 1));  // the wave's first row with a partner
    if (MODE == LD_BLOCK) m1 = (int)min((int64_t)m1, q0 + (tid | 63));                  // below the wave's last lane
    const int self = live ? (int)jq : (MODE == LD_DEGREE ? LD_NONE : -1);
    const uint32_t wq = (MODE == LD_DEGREE && live && w != nullptr) ? w[row] : 1u;
    u64 sum = 0;
    int flag = 0, best = LD_NONE;
    // (one row at a time: interleaving two rows of the counting loop doubles its registers and halves the waves per SIMD)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int m = m0; m < m1; ++m) {
        const int mr = MODE == LD_DEGREE ? m : mlist[m];  // wave-uniform
        const uint32_t* cr = c + (size_t)mr * W32;
        uint32_t inter = 0;
#pragma unroll
        for (int k = 0; k < W32; ++k) inter += __popc(x[k] & cr[k]);
        const uint32_t un = qc + card[mr] - inter;
        const bool hit = inter >= (uint32_t)imin[un];
        if (MODE == LD_DEGREE) {
            if (hit && m > self) {
                sum += w != nullptr ? (u64)w[m] : 1ull;
                flag = 1;
                atomicAdd(&dens[m], (u64)wq);
                atomicOr(&aux[m], 1);
            }
        } else if (MODE == LD_COVER) {
            if (hit && live) flag = 1;
        } else if (MODE == LD_BLOCK) {
            if (hit && m < self && state[mr] == ST_UNDECIDED) flag = 1;
        } else {
            if (hit && live) best = min(best, m);
        }
    }
    if (MODE == LD_DEGREE) {
        if (flag) {
            atomicAdd(&dens[row], sum);
            atomicOr(&aux[row], 1);
        }
    } else if (MODE == LD_COVER) {
        if (flag) atomicOr(&state[row], ST_MEMBER);
    } else if (MODE == LD_BLOCK) {
        if (flag) atomicOr(&aux[row], 1);
    } else {
        if (best != LD_NONE) atomicMin(&aux[row], best);
    }
}

// any width, any alignment: one wave per row, lanes stride over the bytes of every row of the range; every lane holds the
// pair's counts after the wave sums, lane 0 acts
template <int MODE>
__global__ __launch_bounds__(256) void k_ld_pairs_generic(const uint8_t* __restrict__ c, const uint32_t* __restrict__ card,
                                                          int64_t nbytes, double radius, const int* __restrict__ qlist,
                                                          int nq, const int* __restrict__ mlist, int nm, int per,
                                                          const uint32_t* __restrict__ w, u64* dens, int* aux, int* state) {
    const int lane = threadIdx.x & 63;
    const int64_t jq = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (jq >= nq) return;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    int m1 = (int)min((int64_t)nm, r0 + per);
    int m0 = (int)r0;
    if (MODE == LD_DEGREE) m0 = (int)max(r0, jq + 1);
    if (MODE == LD_BLOCK) m1 = (int)min((int64_t)m1, jq);
    if (m0 >= m1) return;
    const int row = MODE == LD_DEGREE ? (int)jq : qlist[jq];
    if (MODE == LD_BLOCK && state[row] != ST_UNDECIDED) return;
    const uint8_t* qr = c + (size_t)row * nbytes;
    const uint32_t qc = card[row];
    const uint32_t wq = (MODE == LD_DEGREE && w != nullptr) ? w[row] : 1u;
    u64 sum = 0;
    int flag = 0, best = LD_NONE;
    for (int m = m0; m < m1; ++m) {
        const int mr = MODE == LD_DEGREE ? m : mlist[m];
        const uint8_t* cr = c + (size_t)mr * nbytes;
        uint32_t inter = 0;
        for (int64_t j = lane; j < nbytes; j += 64) inter += __popc((uint32_t)(qr[j] & cr[j]));
        inter = wave_sum_u32(inter);
        const uint32_t un = qc + card[mr] - inter;
        if (!(jaccard_dist(inter, un) <= radius)) continue;
        if (MODE == LD_DEGREE) {
            sum += w != nullptr ? (u64)w[m] : 1ull;
            flag = 1;
            if (lane == 0) {
                atomicAdd(&dens[m], (u64)wq);
                atomicOr(&aux[m], 1);
            }
        } else if (MODE == LD_COVER) {
            flag = 1;
        } else if (MODE == LD_BLOCK) {
            if (state[mr] == ST_UNDECIDED) flag = 1;
        } else {
            best = min(best, m);
        }
    }
    if (lane != 0) return;
    if (MODE == LD_DEGREE) {
        if (flag) {
            atomicAdd(&dens[row], sum);
            atomicOr(&aux[row], 1);
        }
    } else if (MODE == LD_COVER) {
        if (flag) atomicOr(&state[row], ST_MEMBER);
    } else if (MODE == LD_BLOCK) {
        if (flag) atomicOr(&aux[row], 1);
    } else {
        if (best != LD_NONE) atomicMin(&aux[row], best);
    }
}

// working row p = original row aidx[p], bytes beyond nbytes zero; the state of the rounds starts here
__global__ __launch_bounds__(256) void k_ld_gather(const uint8_t* __restrict__ rows, int64_t nbytes, int64_t wb, int na,
                                                   const int* __restrict__ aidx, const uint32_t* __restrict__ ccard,
                                                   uint8_t* __restrict__ g, uint32_t* __restrict__ gcard,
                                                   int* __restrict__ state, int* __restrict__ blocked,
                                                   int* __restrict__ best, int* __restrict__ ulist) {
    const int64_t total = (int64_t)na * wb;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t p = i / wb, k = i - p * wb;
        const int v = aidx[p];
        g[i] = k < nbytes ? rows[(size_t)v * nbytes + k] : (uint8_t)0;
        if (k == 0) {
            gcard[p] = ccard[v];
            state[p] = ST_UNDECIDED;
            blocked[p] = 0;
            best[p] = LD_NONE;
            ulist[p] = (int)p;
        }
    }
}

// exclusive offsets of two flags over a workgroup of 1024, and their totals; both travel in one int (each sum <= 1024)
__device__ __forceinline__ void ld_scan2(int fa, int fb, int* wsum, int& offa, int& offb, int& tota, int& totb) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mine = fa | (fb << 16);
    int v = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int t = wsum[k];
        before += k < wave ? t : 0;
        all += t;
    }
    const int ex = before + v - mine;
    offa = ex & 0xffff;
    offb = ex >> 16;
    tota = all & 0xffff;
    totb = all >> 16;
    __syncthreads();
}

// One workgroup, after the block pass has ended: an undecided row that nothing blocked becomes a centre (and goes to newc,
// the table of the next cover pass); a blocked one stays in the list, in order, with its mark cleared.  counts = {rows
// still undecided, new centres}.
__global__ __launch_bounds__(1024) void k_ld_round_scan(int nu, const int* __restrict__ uin, int* state, int* blocked,
                                                        int* __restrict__ uout, int* __restrict__ newc,
                                                        int* __restrict__ counts) {
    __shared__ int wsum[16];
    const int tid = (int)threadIdx.x;
    int cu = 0, cc = 0;
    for (int64_t base = 0; base < nu; base += 1024) {
        const int64_t i = base + tid;
        int row = 0, fu = 0, fc = 0;
        if (i < nu) {
            row = uin[i];
            if (state[row] == ST_UNDECIDED) {
                fu = blocked[row] != 0;
                fc = !fu;
            }
        }
        int ou, oc, tu, tc;
        ld_scan2(fu, fc, wsum, ou, oc, tu, tc);
        if (fu) {
            uout[cu + ou] = row;
            blocked[row] = 0;
        }
        if (fc) {
            newc[cc + oc] = row;
            state[row] = ST_CENTRE;
        }
        cu += tu;
        cc += tc;
    }
    if (tid == 0) {
        counts[0] = cu;
        counts[1] = cc;
    }
}

// The tail, one launch per position j of the undecided list, in order.  If that row is still undecided when the launch
// starts it is a centre and every later undecided neighbour becomes a member; else the launch returns at once.  The
// launch never writes state[ulist[j]] (only later entries, each by the one wave that owns it), and what it reads of it was
// stored by earlier launches.  A row that is still undecided when all launches are over is a centre.
__global__ __launch_bounds__(256) void k_ld_step(const uint8_t* __restrict__ g, const uint32_t* __restrict__ gcard,
                                                 int64_t wb, double radius, const int* __restrict__ ulist, int nu, int j,
                                                 int* state) {
    const int v = ulist[j];
    if (state[v] != ST_UNDECIDED) return;
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)j + 1 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= nu) return;
    const int row = ulist[idx];
    if (state[row] != ST_UNDECIDED) return;
    const uint8_t* a = g + (size_t)v * wb;
    const uint8_t* b = g + (size_t)row * wb;
    uint32_t inter = 0;
    for (int64_t k = lane; k < wb; k += 64) inter += __popc((uint32_t)(a[k] & b[k]));
    inter = wave_sum_u32(inter);
    const uint32_t un = gcard[v] + gcard[row] - inter;
    if (lane == 0 && jaccard_dist(inter, un) <= radius) atomicOr(&state[row], ST_MEMBER);
}

// One workgroup, after the tail: the centres and the members of the working table, each in priority order
__global__ __launch_bounds__(1024) void k_ld_final_scan(int na, const int* __restrict__ state, int* __restrict__ clist,
                                                        int* __restrict__ mlist, int* __restrict__ counts) {
    __shared__ int wsum[16];
    const int tid = (int)threadIdx.x;
    int cc = 0, cm = 0;
    for (int64_t base = 0; base < na; base += 1024) {
        const int64_t i = base + tid;
        const int fm = i < na && state[i] == ST_MEMBER;
        const int fc = i < na && !fm;
        int oc, om, tc, tm;
        ld_scan2(fc, fm, wsum, oc, om, tc, tm);
        if (fc) clist[cc + oc] = (int)i;
        if (fm) mlist[cm + om] = (int)i;
        cc += tc;
        cm += tm;
    }
    if (tid == 0) {
        counts[0] = cc;
        counts[1] = cm;
    }
}

// centre[original row] of the working rows; a member's is the centre at position best[] of the list of centres
__global__ __launch_bounds__(256) void k_ld_scatter(int na, int nc, const int* __restrict__ aidx, const int* __restrict__ state,
                                                    const int* __restrict__ best, const int* __restrict__ clist,
                                                    int32_t* __restrict__ centre) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= na) return;
    const int v = aidx[p];
    if (state[p] != ST_MEMBER) centre[v] = v;
    else centre[v] = (unsigned)best[p] < (unsigned)nc ? aidx[clist[best[p]]] : -1;  // (-1: a member without a centre, a bug)
}

// One workgroup (k_cc_scan): rank[v] = the number of centres below row v, and their number
__global__ __launch_bounds__(1024) void k_ld_rank(int n, const int32_t* __restrict__ centre, int* __restrict__ rank,
                                                  int64_t* __restrict__ count) {
    __shared__ int wsum[16];
    const int tid = (int)threadIdx.x;
    int carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const int flag = (i < n && centre[i] == (int)i) ? 1 : 0;
        int off, unused, tot, unused2;
        ld_scan2(flag, 0, wsum, off, unused, tot, unused2);
        if (rank != nullptr && i < n) rank[i] = carry + off;
        carry += tot;
    }
    if (tid == 0 && count != nullptr) *count = carry;
}

__global__ __launch_bounds__(256) void k_ld_label(int n, const int32_t* __restrict__ centre, const int* __restrict__ rank,
                                                  int32_t* __restrict__ label) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int c = centre[v];
    label[v] = (unsigned)c < (unsigned)n ? rank[c] : -1;
}

// one pair pass over a table of `width` bytes per row: lanes qlist[0 .. nq), table side mlist[0 .. nm)
struct Pairs {
    const uint8_t* c;
    const uint32_t* card;
    int64_t width;
    bool fast;
    const uint16_t* tab;
    double radius;
    hipStream_t s;

    template <int MODE>
    int run(const int* qlist, int64_t nq, const int* mlist, int64_t nm, const uint32_t* w, u64* dens, int* aux, int* state) const {
        if (nq <= 0 || nm <= 0) return BBH_OK;
        int64_t qblocks = 0;
        int per = 0, nsplit = 0;
        radius_ranges(nq, nm, fast, LD_FILL, &qblocks, &per, &nsplit);
        const dim3 grid((unsigned)qblocks, (unsigned)nsplit);
#define BB_LAUNCH_LD(W)                                                                                                   \
    hipLaunchKernelGGL((k_ld_pairs<W, MODE>), grid, dim3(256), 0, s, (const uint32_t*)c, card, tab, qlist, (int)nq, mlist, \
                       (int)nm, per, w, dens, aux, state)
        if (!fast)
            hipLaunchKernelGGL((k_ld_pairs_generic<MODE>), grid, dim3(256), 0, s, c, card, width, radius, qlist, (int)nq, mlist,
                               (int)nm, per, w, dens, aux, state);
        else if (width == 8) BB_LAUNCH_LD(2);
        else if (width == 16) BB_LAUNCH_LD(4);
        else if (width == 32) BB_LAUNCH_LD(8);
        else if (width == 64) BB_LAUNCH_LD(16);
        else if (width == 128) BB_LAUNCH_LD(32);
        else BB_LAUNCH_LD(64);
#undef BB_LAUNCH_LD
        BB_HIP(hipGetLastError());
        return BBH_OK;
    }
};

// BBHIP_LEADERS_ROUNDS, read at every call: k >= 0 forces the tail after k rounds, anything else is the built-in rule
int forced_rounds() {
    const char* e = std::getenv("BBHIP_LEADERS_ROUNDS");
    if (e == nullptr || *e == '\0') return -1;
    char* end = nullptr;
    const long v = std::strtol(e, &end, 10);
    return (end == e || *end != '\0' || v < 0 || v > 0x7fffffffL) ? -1 : (int)v;
}

}  // namespace

extern "C" int bbh_jt_leaders(const uint8_t* rows, int64_t n, int64_t nbytes, double radius, const uint32_t* weights,
                              uint32_t flags, int32_t* out_centre, int32_t* out_label, int64_t* out_count,
                              uint64_t* out_density, void* stream) {
    BB_TRY(bb::ensure_device());
    if (n < 0 || n > 0x7fffffffLL || nbytes <= 0) return bb::fail(BBH_ERR_INVALID, "leaders: need 0 <= n < 2^31 and nbytes > 0");
    if (radius != radius) return bb::fail(BBH_ERR_INVALID, "leaders: the radius is NaN");
    if ((flags & ~BBH_LEADERS_TIES_HIGH) != 0u) return bb::fail(BBH_ERR_INVALID, "leaders: unknown flag bits 0x%x", flags);
    if (out_centre == nullptr && out_label == nullptr && out_count == nullptr && out_density == nullptr)
        return bb::fail(BBH_ERR_INVALID, "leaders: need a centre, a label, a count or a density output");
    if (n > 0 && rows == nullptr) return bb::fail(BBH_ERR_INVALID, "leaders: no rows");
    const bool ties_high = (flags & BBH_LEADERS_TIES_HIGH) != 0u;
    hipStream_t s = (hipStream_t)stream;
    bb::DevIn c, win;
    bb::DevOut oce, ol, oc, od;
    BB_TRY(oc.init(out_count, 8));
    bb::DevScope tmp(s);
    if (n == 0) {
        if (oc.dev) BB_HIP(hipMemsetAsync(oc.dev, 0, 8, s));
        BB_TRY(oc.finish(s));
        return tmp.sync();
    }
    BB_TRY(oce.init(out_centre, (size_t)n * 4));
    BB_TRY(ol.init(out_label, (size_t)n * 4));
    BB_TRY(od.init(out_density, (size_t)n * 8));
    BB_TRY(c.init(rows, (size_t)(n * nbytes), s));
    BB_TRY(win.init(weights, (size_t)n * 4, s));
    const uint8_t* cd = (const uint8_t*)c.dev;
    const uint32_t* w = (const uint32_t*)win.dev;

    uint32_t* ccard = nullptr;
    u64* dens = (u64*)od.dev;
    int32_t* centre = (int32_t*)oce.dev;
    int* mark = nullptr;  // "has a neighbour"; after the degree pass is read, the ranks of the centres
    BB_HIP(tmp.get(&ccard, (size_t)n * 4));
    BB_HIP(tmp.get(&mark, (size_t)n * 4));
    if (dens == nullptr) BB_HIP(tmp.get(&dens, (size_t)n * 8));
    if (centre == nullptr) BB_HIP(tmp.get(&centre, (size_t)n * 4));
    const dim3 flat((unsigned)((n + 255) / 256));

    if (radius >= 1.0) {
        // (u - i) / u lies in [0, 1]: every row is every row's neighbour, all densities are equal, the tie rule picks
        bb::ProfScope ps("jt_leaders/degree", s);
        ps.units(n);
        u64* total = nullptr;
        BB_HIP(tmp.get(&total, 8));
        hipLaunchKernelGGL(k_ld_total, dim3(1), dim3(1024), 0, s, (int)n, w, total);
        BB_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ld_fill_all, flat, dim3(256), 0, s, (int)n, total, ties_high ? (int)(n - 1) : 0, dens, centre);
        BB_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_ld_init, flat, dim3(256), 0, s, (int)n, w, dens, mark, centre);
        BB_HIP(hipGetLastError());
    }
    if (radius >= 0.0 && radius < 1.0) {
        // the width of the working table: rows of up to 256 bytes are zero-padded to the next instantiated width
        int64_t wb = nbytes;
        if (nbytes <= 256) {
            wb = 8;
            while (wb < nbytes) wb *= 2;
        }
        const bool wfast = nbytes <= 256;
        const bool fast = (uintptr_t)cd % 4 == 0 && radius_fast_width(nbytes);
        uint16_t* tab = nullptr;
        if (wfast) {
            const int nbits = (int)wb * 8;
            BB_HIP(tmp.get(&tab, (size_t)(nbits + 1) * 2));
            hipLaunchKernelGGL(k_radius_table, dim3((unsigned)(nbits / 256 + 1)), dim3(256), 0, s, radius, nbits, tab);
            BB_HIP(hipGetLastError());
        }
        // 1. degrees
        BB_TRY(bbh_popcount_rows(cd, n, nbytes, nbytes, ccard, s));
        {
            bb::ProfScope ps("jt_leaders/degree", s);
            ps.units(n);
            const Pairs orig{cd, ccard, nbytes, fast, tab, radius, s};
            BB_TRY(orig.run<LD_DEGREE>(nullptr, n, nullptr, n, w, dens, mark, nullptr));
        }
        // 2., 3. the rows with a neighbour, by priority; the others are done: their own centres
        std::vector<u64> hdens((size_t)n);
        std::vector<int> hmark((size_t)n);
        BB_HIP(hipMemcpyAsync(hdens.data(), dens, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        BB_HIP(hipMemcpyAsync(hmark.data(), mark, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        BB_TRY(tmp.sync());
        std::vector<int> act;
        for (int64_t v = 0; v < n; ++v)
            if (hmark[(size_t)v] != 0) act.push_back((int)v);
        hmark = std::vector<int>();
        const u64* hd = hdens.data();
        if (ties_high)
            std::sort(act.begin(), act.end(), [hd](int a, int b) { return hd[a] != hd[b] ? hd[a] > hd[b] : a > b; });
        else
            std::sort(act.begin(), act.end(), [hd](int a, int b) { return hd[a] != hd[b] ? hd[a] > hd[b] : a < b; });
        hdens = std::vector<u64>();
        const int64_t na = (int64_t)act.size();
        if (na > 0) {
            int *aidx = nullptr, *state = nullptr, *blocked = nullptr, *best = nullptr, *ua = nullptr, *ub = nullptr,
                *newc = nullptr, *counts = nullptr;
            uint8_t* g = nullptr;
            uint32_t* gcard = nullptr;
            BB_HIP(tmp.get(&aidx, (size_t)na * 4));
            BB_HIP(tmp.get(&state, (size_t)na * 4));
            BB_HIP(tmp.get(&blocked, (size_t)na * 4));
            BB_HIP(tmp.get(&best, (size_t)na * 4));
            BB_HIP(tmp.get(&ua, (size_t)na * 4));
            BB_HIP(tmp.get(&ub, (size_t)na * 4));
            BB_HIP(tmp.get(&newc, (size_t)na * 4));
            BB_HIP(tmp.get(&gcard, (size_t)na * 4));
            BB_HIP(tmp.get(&counts, 8));
            BB_HIP(tmp.get(&g, (size_t)na * (size_t)wb));
            BB_HIP(hipMemcpyAsync(aidx, act.data(), (size_t)na * 4, hipMemcpyHostToDevice, s));
            const int64_t gblocks = std::min<int64_t>((na * wb + 255) / 256, 1 << 20);
            hipLaunchKernelGGL(k_ld_gather, dim3((unsigned)gblocks), dim3(256), 0, s, cd, nbytes, wb, (int)na, aidx, ccard, g,
                               gcard, state, blocked, best, ua);
            BB_HIP(hipGetLastError());
            const Pairs work{g, gcard, wb, wfast, tab, radius, s};
            int hcounts[2] = {0, 0};
            // 4. rounds
            const int forced = forced_rounds();
            int64_t nu = na, ncn = 0, before_last = -1;  // before_last: the rows undecided before the round before
            int rounds = 0;
            while (nu > 0) {
                if (forced >= 0 ? rounds >= forced : rounds >= LD_ROUND_CAP) break;
                bb::ProfScope ps("jt_leaders/round", s);
                ps.units(nu);
                BB_TRY(work.run<LD_COVER>(ua, nu, newc, ncn, nullptr, nullptr, nullptr, state));
                BB_TRY(work.run<LD_BLOCK>(ua, nu, ua, nu, nullptr, nullptr, blocked, state));
                hipLaunchKernelGGL(k_ld_round_scan, dim3(1), dim3(1024), 0, s, (int)nu, ua, state, blocked, ub, newc, counts);
                BB_HIP(hipGetLastError());
                BB_HIP(hipMemcpyAsync(hcounts, counts, 8, hipMemcpyDeviceToHost, s));
                BB_TRY(tmp.sync());
                ++rounds;
                const int64_t left = hcounts[0];
                ncn = hcounts[1];
                if (left < 0 || left >= nu || ncn < 0 || ncn > nu)  // (the first undecided row is covered or never blocked)
                    return bb::fail(BBH_ERR_STATE, "leaders: round %d decided nothing (%lld rows undecided)", rounds, (long long)nu);
                std::swap(ua, ub);
                // the built-in rule (measured in DESIGN.md 5i): two consecutive rounds that together decided less than 1 / 64 of
                // the rows undecided before them are walking a chain; step from here.  (Random graphs start slowly - 7 % in the
                // first two rounds - and then fall geometrically; a chain decides two rows a round for ever.)
                const bool slow = before_last >= 0 && (before_last - left) * LD_SLOW < before_last;
                before_last = nu;
                nu = left;
                if (forced < 0 && slow) break;
            }
            // 5. the tail
            if (nu > 0) {
                bb::ProfScope ps("jt_leaders/step", s);
                ps.units(nu);
                BB_TRY(work.run<LD_COVER>(ua, nu, newc, ncn, nullptr, nullptr, nullptr, state));  // owed to the last round's centres
                for (int64_t j = 0; j < nu; ++j) {
                    const int64_t later = nu - 1 - j;
                    hipLaunchKernelGGL(k_ld_step, dim3((unsigned)std::max<int64_t>(1, (later + 3) / 4)), dim3(256), 0, s, g, gcard,
                                       wb, radius, ua, (int)nu, (int)j, state);
                    BB_HIP(hipGetLastError());
                }
            }
            // 6. every member's highest-priority neighbouring centre
            {
                bb::ProfScope ps("jt_leaders/assign", s);
                int *clist = ub, *mlist = newc;  // (the lists of the rounds are done with once the tail has run)
                hipLaunchKernelGGL(k_ld_final_scan, dim3(1), dim3(1024), 0, s, (int)na, state, clist, mlist, counts);
                BB_HIP(hipGetLastError());
                BB_HIP(hipMemcpyAsync(hcounts, counts, 8, hipMemcpyDeviceToHost, s));
                BB_TRY(tmp.sync());
                const int64_t ncl = hcounts[0], nm = hcounts[1];
                ps.units(nm);
                BB_TRY(work.run<LD_ASSIGN>(mlist, nm, clist, ncl, nullptr, nullptr, best, nullptr));
                hipLaunchKernelGGL(k_ld_scatter, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, s, (int)na, (int)ncl, aidx, state,
                                   best, clist, centre);
                BB_HIP(hipGetLastError());
            }
        }
    }
    // 7. labels: the rank of the centre among the centres in ascending row index
    if (ol.dev != nullptr || oc.dev != nullptr) {
        int* rank = ol.dev != nullptr ? mark : nullptr;
        hipLaunchKernelGGL(k_ld_rank, dim3(1), dim3(1024), 0, s, (int)n, centre, rank, (int64_t*)oc.dev);
        BB_HIP(hipGetLastError());
    }
    if (ol.dev != nullptr) {
        hipLaunchKernelGGL(k_ld_label, flat, dim3(256), 0, s, (int)n, centre, mark, (int32_t*)ol.dev);
        BB_HIP(hipGetLastError());
    }
    BB_TRY(oce.finish(s));
    BB_TRY(ol.finish(s));
    BB_TRY(oc.finish(s));
    BB_TRY(od.finish(s));
    return tmp.sync();
}
