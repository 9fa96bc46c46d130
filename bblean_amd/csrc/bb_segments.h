// bb_segments.h -- what the segmented kernels share: k independent sets of packed rows in one call
// (bb_medoid.hip: complementary iSIM and medoids; bb_cluster_stats.hip: centroids, iSIM, distances, column sums).
// How a set's rows are addressed, the bit-sliced column counter, the column-sum kernel of the large path, the index
// check of a device-resident `members`, and the argument checks of the two entry points.  Everything is in an unnamed
// namespace: each translation unit that includes this header gets its own copy of the kernels.
#pragma once

#include "bb_common.h"

namespace {

using namespace bbd;

// Largest set a one-wave kernel takes: 2^11 - 1 rows = 11 planes in registers per word.  Chosen by reasoning, not
// measured.
constexpr int SMALL_PLANES = 11;
constexpr int64_t SMALL_MAX = (1 << SMALL_PLANES) - 1;
constexpr int CHUNK = 256;      // rows per wave in the kernels of the large path
constexpr int CHUNK_PLANES = 9; // a chunk's counts are <= 256 < 2^9
constexpr int MAX_WORDS_REG = 128;  // rows of up to 512 bytes keep their planes in registers

__device__ __forceinline__ uint32_t ld_word(const uint8_t* row, int w, int nb, bool al) {
    const int o = w * 4;
    if (o >= nb) return 0u;
    if (al && o + 4 <= nb) return *reinterpret_cast<const uint32_t*>(row + o);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (o + k < nb) v |= (uint32_t)row[o + k] << (8 * k);
    return v;
}

// sum over the wave as a wave-uniform value
__device__ __forceinline__ uint32_t wave_total(uint32_t v) {
    v = row16_sum(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

struct Rows {  // how the rows of a set are addressed
    const uint8_t* base;
    int64_t stride;
    const int64_t* members;  // NULL: set order = row order
    int nb;                  // used bytes of a row (n_features / 8)
    bool al;                 // rows start at 4-byte boundaries
    __device__ __forceinline__ const uint8_t* row(int64_t flat) const {
        const int64_t r = members ? members[flat] : flat;  // (validated before any kernel that dereferences it)
        return base + r * stride;
    }
};

template <int WPL, int NP>
__device__ __forceinline__ void planes_add(uint32_t (&P)[WPL][NP], const uint32_t (&x)[WPL]) {
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
        uint32_t carry = x[j];
#pragma unroll
        for (int b = 0; b < NP; ++b) {
            const uint32_t t = P[j][b] & carry;
            P[j][b] ^= carry;
            carry = t;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Large path, one set per sequence of launches.  Counters: cnt[t * n_words + w] = count of bit t of word w.
// ---------------------------------------------------------------------------------------------------------------
// a wave adds a chunk of rows bit-sliced, 64 words at a time, and flushes the chunk's counts with integer atomics
__global__ __launch_bounds__(256) void k_seg_colsum(Rows R, int64_t beg, int64_t m, int n_words,
                                                    uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t i0 = uniform_i64(((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * CHUNK);
    if (i0 >= m) return;
    const int64_t i1 = i0 + CHUNK < m ? i0 + CHUNK : m;
    for (int w0 = 0; w0 < n_words; w0 += 64) {
        uint32_t P[1][CHUNK_PLANES];
#pragma unroll
        for (int b = 0; b < CHUNK_PLANES; ++b) P[0][b] = 0;
        for (int64_t i = i0; i < i1; i += 4) {
            uint32_t x[4][1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = i + j < i1;
                const uint32_t v = ld_word(R.row(beg + (ok ? i + j : i1 - 1)), w0 + lane, R.nb, R.al);
                x[j][0] = ok ? v : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) planes_add<1, CHUNK_PLANES>(P, x[j]);
        }
        if (w0 + lane < n_words) {
#pragma unroll
            for (int t = 0; t < 32; ++t) {
                uint32_t c = 0;
#pragma unroll
                for (int b = 0; b < CHUNK_PLANES; ++b) c |= ((P[0][b] >> t) & 1u) << b;
                if (c) atomicAdd(&cnt[(size_t)t * n_words + w0 + lane], c);
            }
        }
    }
}

// flag = 1 when an entry of a device-resident `members` is not a row
__global__ __launch_bounds__(256) void k_seg_check(const int64_t* __restrict__ members, int64_t total, int64_t n_rows,
                                                   int* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = members[i];
        bad |= r < 0 || r >= n_rows;
    }
    if (bad) *flag = 1;
}

int seg_cu_count() {
    static int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;
        return v;
    }();
    return n;
}

int bit_length(int64_t v) {
    int n = 0;
    while (v > 0) {
        ++n;
        v >>= 1;
    }
    return n;
}

// ---------------------------------------------------------------------------------------------------------------
// The argument checks of a segmented entry point, in the order bbh_compl_isim_segments has always made them, and what
// they find out on the way.  `what` starts every message.  Nothing is written before all of them have passed.
// ---------------------------------------------------------------------------------------------------------------
struct SegPlan {
    std::vector<int64_t> off_host;  // a device-resident `offsets`, copied
    const int64_t* off = nullptr;   // the offsets on the host
    int n_words = 0;
    bool regs = false;              // the planes of a row fit the registers
    int64_t small_max = 0;          // sets of up to this many rows are the one-wave kernel's
    int64_t small_rows = 0, n_small = 0, large_rows = 0, n_large = 0, largest = 0, total = 0;
};

// the scalar arguments, then the offsets: which sets go where (`small_max_wide`: small_max for rows beyond the registers)
inline int seg_plan_offsets(const char* what, const uint8_t* rows, int64_t n_rows, int64_t nbytes, int64_t row_stride,
                            const int64_t* members, const int64_t* offsets, int64_t k, int64_t n_features,
                            int64_t small_max_wide, hipStream_t s, SegPlan& p) {
    if (rows == nullptr || offsets == nullptr || n_rows < 1 || nbytes <= 0 || row_stride < nbytes || k < 1)
        return bb::fail(BBH_ERR_INVALID, "%s: need rows, offsets, n_rows >= 1, k >= 1 and row_stride >= nbytes", what);
    if (n_features <= 0 || n_features % 8 != 0 || n_features > nbytes * 8)
        return bb::fail(BBH_ERR_INVALID, "Only n_features divisible by 8 is supported");
    // offsets are needed on the host (which sets go where), so a device-resident array is copied and checked here too
    p.off = offsets;
    if (bb::is_device_ptr(offsets)) {
        p.off_host.resize((size_t)k + 1);
        BB_HIP(hipMemcpyAsync(p.off_host.data(), offsets, (size_t)(k + 1) * 8, hipMemcpyDeviceToHost, s));
        BB_HIP(hipStreamSynchronize(s));
        p.off = p.off_host.data();
    }
    const int64_t* off = p.off;
    if (off[0] != 0) return bb::fail(BBH_ERR_INVALID, "%s: offsets must start at 0", what);
    p.n_words = (int)((n_features / 8 + 3) / 4);
    p.regs = p.n_words <= MAX_WORDS_REG;
    p.small_max = p.regs ? SMALL_MAX : small_max_wide;
    for (int64_t g = 0; g < k; ++g) {
        const int64_t m = off[g + 1] - off[g];
        if (m < 0) return bb::fail(BBH_ERR_INVALID, "%s: offsets must not decrease", what);
        if (m == 0) return bb::fail(BBH_ERR_INVALID, "%s: set %lld is empty", what, (long long)g);
        // Q <= n_features * m^2 and (m - 1) * S <= n_features * m^2 must fit uint64
        if (m >= (1ll << 31) || m * m > 0x7fffffffffffffffll / n_features)
            return bb::fail(BBH_ERR_INVALID, "%s: set %lld has %lld rows, n_features * m * m must stay below 2^63", what,
                            (long long)g, (long long)m);
        if (m <= p.small_max) {
            p.small_rows += m;
            ++p.n_small;
        } else {
            p.large_rows += m;
            ++p.n_large;
            if (m > p.largest) p.largest = m;
        }
    }
    p.total = off[k];
    if (members == nullptr && p.total > n_rows)
        return bb::fail(BBH_ERR_INVALID, "%s: offsets name %lld rows, there are %lld", what, (long long)p.total,
                        (long long)n_rows);
    if (members != nullptr && !bb::is_device_ptr(members)) {
        for (int64_t i = 0; i < p.total; ++i)
            if (members[i] < 0 || members[i] >= n_rows)
                return bb::fail(BBH_ERR_INVALID, "%s: members[%lld] = %lld is not a row", what, (long long)i,
                                (long long)members[i]);
    }
    return BBH_OK;
}

// a device-resident `members` is checked by a kernel (tmp's stream is synchronised)
inline int seg_check_members_dev(const char* what, const int64_t* members, int64_t total, int64_t n_rows, hipStream_t s,
                                 bb::DevScope& tmp) {
    int* flag = nullptr;
    BB_HIP(tmp.get(&flag, 4));
    BB_HIP(hipMemsetAsync(flag, 0, 4, s));
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_seg_check, dim3((unsigned)blocks), dim3(256), 0, s, members, total, n_rows, flag);
    BB_HIP(hipGetLastError());
    int bad = 0;
    BB_HIP(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, s));
    BB_TRY(tmp.sync());
    if (bad) return bb::fail(BBH_ERR_INVALID, "%s: an entry of members is not a row", what);
    return BBH_OK;
}

}  // namespace
