// bb_radius_common.h -- what the callers of "within a Jaccard distance" share (bb_radius.hip, bb_components.hip): the
// distance, the table of smallest passing intersections and the rule that splits a table into ranges.  DESIGN.md 5f, 5h.
// Everything is in an unnamed namespace: each translation unit gets its own copy.
#pragma once

#include "bb_common.h"

namespace {

// bbh_jt_dist_matrix's value: one float64 division of the exact counts, 0.0 where the union is empty
__device__ __forceinline__ double jaccard_dist(uint32_t inter, uint32_t un) {
    return un == 0u ? 0.0 : (double)(un - inter) / (double)un;
}

// imin[u] for u = 0 .. nbits: bisection on the monotone predicate jaccard_dist(i, u) <= radius
__global__ __launch_bounds__(256) void k_radius_table(double radius, int nbits, uint16_t* __restrict__ tab) {
    const int u = (int)(blockIdx.x * 256 + threadIdx.x);
    if (u > nbits) return;
    int lo = 0, hi = u + 1;  // the answer lies in [lo, hi]; hi = u + 1 is "none"
    if (jaccard_dist((uint32_t)u, (uint32_t)u) <= radius) {
        hi = u;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (jaccard_dist((uint32_t)mid, (uint32_t)u) <= radius) hi = mid;
            else lo = mid + 1;
        }
    }
    tab[u] = (uint16_t)hi;
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

// the widths the lane-per-query kernels are instantiated for; everything else, and every unaligned operand, is generic
inline bool radius_fast_width(int64_t nbytes) {
    return nbytes == 8 || nbytes == 16 || nbytes == 32 || nbytes == 64 || nbytes == 128 || nbytes == 256;
}

// The ranges of bbh_jt_assign: fill the device `fill` times over (bbh_jt_assign's and bbh_jt_radius's 4), with at least 64
// rows per range.  qblocks = workgroups along the queries (tiles of 256, or four waves of one query each in the generic
// kernels).
inline void radius_ranges(int64_t nq, int64_t nc, bool fast, int fill, int64_t* qblocks, int* per, int* nsplit) {
    *qblocks = fast ? (nq + 255) / 256 : (nq + 3) / 4;
    int64_t want = ((int64_t)fill * cu_count() + *qblocks - 1) / *qblocks;
    const int64_t most = (nc + 63) / 64;
    if (want > most) want = most;
    if (want > 65535) want = 65535;
    *per = (int)((nc + want - 1) / want);
    *nsplit = (int)((nc + *per - 1) / *per);
}

}  // namespace
