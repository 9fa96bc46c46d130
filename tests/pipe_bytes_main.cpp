// Host walk through bblean_amd/csrc/bb_pipe_bytes.h (tests/test_pipe_bytes.py builds and runs it): one "PASS name" or "FAIL name ..."
// line per check.  The references are the scalar definitions and the kernel's former byte-at-a-time loops, written out here.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../bblean_amd/csrc/bb_pipe_bytes.h"

// v_alignbit_b32(a, b, s): the low dword of {a, b} >> s
static uint32_t alignbit(uint32_t a, uint32_t b, uint32_t s) { return (uint32_t)(((((uint64_t)a) << 32) | b) >> s); }
static uint32_t bitreverse32(uint32_t x) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i);
    return r;
}
// bb_tree_pipe.inc: bit of feature i of the lane's 32 in its dword of a packed row
static uint32_t xbit(uint32_t xd, int i) { return (xd >> (8 * (i >> 3) + 7 - (i & 7))) & 1u; }
// bb_tree_pipe.inc, centroid_dword31: bit = v >= ceil(n / 2), one alignbit per feature
static uint32_t centroid_dword31(const uint32_t (&v)[32], uint32_t n) {
    const uint32_t hm1 = ((n + 1u) >> 1) - 1u;
    uint32_t out = 0;
    for (int b = 0; b < 4; ++b) {
        uint32_t byte = 0;
        for (int q = 0; q < 8; ++q) byte = alignbit(byte, hm1 - v[8 * b + q], 31);
        out |= (byte & 0xFFu) << (8 * b);
    }
    return out;
}

static int report(const char* name, unsigned long long bad, unsigned long long first) {
    if (bad == 0) printf("PASS %s\n", name);
    else printf("FAIL %s %llu differences, first at %llx\n", name, bad, first);
    return bad != 0;
}

int main() {
    int failed = 0;
    {
        // every pair of neighbouring bytes (the one a borrow would come from / go to) x every threshold, at the three positions
        // a pair can take, the other two bytes at 0 and at 255
        unsigned long long bad = 0, first = 0;
        for (uint32_t k = 1; k <= 128; ++k)
            for (uint32_t lo = 0; lo < 256; ++lo)
                for (uint32_t hi = 0; hi < 256; ++hi)
                    for (int pos = 0; pos < 3; ++pos)
                        for (uint32_t fill = 0; fill < 256; fill += 255) {
                            uint32_t by[4] = {fill, fill, fill, fill};
                            by[pos] = lo; by[pos + 1] = hi;
                            const uint32_t w = by[0] | (by[1] << 8) | (by[2] << 16) | (by[3] << 24);
                            uint32_t want = 0;
                            for (int m = 0; m < 4; ++m) want |= (by[m] >= k ? 0x80u : 0u) << (8 * m);
                            if (bbp_vote4(w, k) != want) { if (!bad++) first = ((unsigned long long)k << 32) | w; }
                        }
        failed += report("vote4_exhaustive", bad, first);
    }
    {
        // every nibble pair (a byte of the packed row) at every byte of the dword: byte m of dword u = feature 4 u + m
        unsigned long long bad = 0, first = 0;
        for (int b = 0; b < 4; ++b)
            for (uint32_t v = 0; v < 256; ++v)
                for (uint32_t fill = 0; fill < 2; ++fill) {
                    const uint32_t xd = ((fill ? 0xFFFFFFFFu : 0u) & ~(0xFFu << (8 * b))) | (v << (8 * b));
                    const uint32_t xr = bitreverse32(xd);
                    for (int u = 0; u < 8; ++u) {
                        uint32_t want = 0;
                        for (int m = 0; m < 4; ++m) want |= xbit(xd, 4 * u + m) << (8 * m);
                        if (bbp_expand_dword(xr, u) != want) { if (!bad++) first = ((unsigned long long)u << 32) | xd; }
                    }
                }
        failed += report("expand_all_nibble_pairs", bad, first);
    }
    {
        // every combination of the eight flags of a byte: feature 8 b + q at bit 7 - q
        unsigned long long bad = 0, first = 0;
        for (uint32_t f = 0; f < 256; ++f) {
            uint32_t fe = 0, fo = 0, want = 0;
            for (int q = 0; q < 8; ++q)
                if ((f >> q) & 1u) {
                    (q < 4 ? fe : fo) |= 0x80u << (8 * (q & 3));
                    want |= 1u << (7 - q);
                }
            if (bbp_gather8(fe, fo) != want) { if (!bad++) first = f; }
        }
        failed += report("gather_all_nibble_pairs", bad, first);
    }
    {
        // the composed dword against centroid_dword31: every n the uint8 tier can have after a merge, counters 0 .. n at random,
        // on and next to the vote threshold, all-equal
        unsigned long long bad = 0, first = 0;
        std::mt19937 rng(12345);
        for (uint32_t n = 2; n <= 255; ++n) {
            const uint32_t k = (n + 1u) >> 1;
            for (int rep = 0; rep < 400; ++rep) {
                uint32_t v[32], w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int i = 0; i < 32; ++i) {
                    const uint32_t r = rng();
                    if (rep < 200) v[i] = r % (n + 1u);
                    else if (rep < 300) v[i] = k - 1u + (r % 3u) > n ? n : k - 1u + (r % 3u);
                    else v[i] = (r & 1u) ? (rep & 1 ? n : k) : (rep & 2 ? 0u : k - 1u);
                    w[i >> 2] |= v[i] << (8 * (i & 3));
                }
                if (bbp_centroid_dword8(w, k) != centroid_dword31(v, n)) { if (!bad++) first = n; }
            }
        }
        failed += report("dword_against_centroid_dword31", bad, first);
    }
    return failed ? 1 : 0;
}
