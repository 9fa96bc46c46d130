// Dword-level helpers of the pipelined kernel's packed (uint8) merge path: four cluster-feature bytes at a time.
// Plain integer code that compiles on the host as well (tests/pipe_bytes_main.cpp walks it exhaustively without a GPU).
//
// A lane holds 32 consecutive features of a BitFeature's linear sum as eight dwords w[0..7]: feature 4 u + m is byte m of
// w[u].  The same 32 features of a packed row are one dword in which feature 8 b + q is bit 8 b + 7 - q (xbit, bb_tree_pipe.inc).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BBP_FN __host__ __device__ __forceinline__
#else
#define BBP_FN static inline
#endif

// nibble (bit m = feature m of four adjacent ones) -> one 0 / 1 byte per feature, byte m = bit m: n * (1 + 2^7 + 2^14 + 2^21)
// puts bit k of n at the bits k + 7 j, of which 8 m is hit by k = j = m only
BBP_FN uint32_t bbp_expand4(uint32_t nibble) { return ((nibble & 15u) * 0x204081u) & 0x01010101u; }

// the eight 0 / 1-byte dwords of a packed row's dword xd, in the order of w[]: xr = xd bit-reversed holds feature 8 b + q at
// bit 24 - 8 b + q, so the features 4 u .. 4 u + 3 are the nibble at bit 24 - 8 (u >> 1) + 4 (u & 1)
BBP_FN uint32_t bbp_expand_dword(uint32_t xr, int u) { return bbp_expand4(xr >> (24 - 8 * (u >> 1) + 4 * (u & 1))); }

// bit 7 of every byte: byte >= k, for 1 <= k <= 128.  The low seven bits of a byte plus 128 minus k stay within 0 .. 254: no
// borrow leaves the byte, and bit 7 of the difference says low7 >= k; a byte of 128 or more is >= k anyway (its own bit 7).
BBP_FN uint32_t bbp_vote4(uint32_t w, uint32_t k) {
    return ((((w & 0x7F7F7F7Fu) | 0x80808080u) - k * 0x01010101u) | w) & 0x80808080u;
}

// one centroid byte from the vote flags of its eight features: fe = flags of the features 8 b .. 8 b + 3 (bbp_vote4 of
// w[2 b]), fo = those of 8 b + 4 .. 8 b + 7 (w[2 b + 1]).  Feature 8 b + q belongs at bit 7 - q.  With the even dword's flags
// moved to the bits 8 m + 4 and the odd one's to 8 m, the multiplier 2^27 + 2^18 + 2^9 + 1 sends bit 8 m + 4 to 31 - m and
// bit 8 m to 27 - m (the term 2^(27 - 9 m)); every other product term lands on a bit of its own below 24 or beyond 31
// (0 4 8 9 12 13 16 17 18 20 21 22), so nothing carries into the top byte.
BBP_FN uint32_t bbp_gather8(uint32_t fe, uint32_t fo) { return (((fe >> 3) | (fo >> 7)) * 0x08040201u) >> 24; }

// new centroid dword of the lane from its eight dwords of uint8 sums: bit = sum >= k, k = ceil(n / 2) <= 128
// (centroid_dword31 on the same 32 values with n = new_n <= 255)
BBP_FN uint32_t bbp_centroid_dword8(const uint32_t (&w)[8], uint32_t k) {
    return bbp_gather8(bbp_vote4(w[0], k), bbp_vote4(w[1], k)) | (bbp_gather8(bbp_vote4(w[2], k), bbp_vote4(w[3], k)) << 8) |
           (bbp_gather8(bbp_vote4(w[4], k), bbp_vote4(w[5], k)) << 16) | (bbp_gather8(bbp_vote4(w[6], k), bbp_vote4(w[7], k)) << 24);
}
