// bb_tree_fast.inc -- the steady-state insertion kernel (2048-bit rows), included by bb_tree.hip.
//
// k_tree_insert (bb_tree.hip) is the complete engine: every shape, every criterion, splits, tier promotions,
// empty trees.  It spends ~2 300 instructions per wave and insert, because one instruction stream carries all of
// that state.  This file is the same algorithm (SURVEY.md Appendix B; reference bitbirch.py:305-357, :488-526)
// restricted to what an insertion does 98 % of the time and written against an instruction budget:
//
//   * every node of the current root-to-leaf path lives in an LDS slot: packed centroids (272-byte row stride),
//     popcounts, links and the 32-byte RowMeta image of every row.  A slot is filled from HBM when the path
//     changes; all updates are written through to HBM, so HBM is always current and the cold paths (below) need
//     no flush.  Nodes whose centroids are all zero (the upper levels of trees over weakly clustered data) keep
//     only a tag: every similarity is 0 and np.argmax returns row 0 (bitbirch.py:320).
//   * node compare: one row per lane, a quarter of the row per wave; the four partial intersections meet through
//     8 bytes of LDS per row and one LDS-only barrier.  The first-argmax is NOT a butterfly of exact fraction
//     compares: each lane forms the correctly rounded float32 quotient inter/union, whose bit pattern orders
//     exactly like the fraction for unions <= 4096 (distinct fractions differ by >= 2^-24 >= 1 ulp and none is a
//     rounding midpoint; equal fractions give equal quotients; tests/test_fast_key.py checks all 6.3 M
//     fractions), so the reduction is six v_max_u32 DPP steps, a ballot and a find-first-set.  Nodes of more than
//     64 rows (bf 254): one WHOLE row per lane (wave w owns rows 64 w ..), the element's row read from LDS, one
//     candidate per wave and a pick among the four behind the barrier.
//   * leaf test + every ancestor's update in one pass (one thread per 8 features) and ONE block reduction whose
//     record is 16-32 bytes per wave (dot product + 16-bit popcount fields, DPP to lane 63).
//   * level state (tags, lengths, row-0 data of tag-only levels) is wave-uniform data parked in VGPRs and read
//     with v_readfirstlane: the scalar register file holds only pointers and counters, nothing spills.
//   * a leaf that overflows while its parent has room is split where it lies: the loop appends the element, leaves
//     with its level records in LDS, tree_fast_body calls cold_leaf_split (the complete engine's split_node on the
//     leaf's slot) and re-enters the loop with the levels above still resident.
//   * anything else - root or cascading splits, the first element of a tree, a tier promotion, clusters of 2^31
//     members, a path deeper than FMAXLV levels - is handed, BEFORE any state is modified, to the complete engine
//     compiled as an out-of-line function (tree_insert_body<.., ONE>), which inserts that one element from HBM;
//     the slots are refilled afterwards.  The cold functions' LDS scratch overlays the last slots.  No call sits
//     inside the insertion loop itself (fast_run): nothing but a few scalars is live across one.
//
// Results are bit-identical to k_tree_insert by construction (same decisions on the same exact integers and the
// same float64 formulae); tests/test_hip_tree.py and tests/test_scale_golden.py run through this kernel.

constexpr int FMAXLV = 7;           // levels of a root-to-leaf path handled here (6 tracking levels + the leaf)
constexpr int FMAXT = FMAXLV - 1;
constexpr uint32_t F_LEAF = 1u, F_ZERO = 2u, F_NOSLOT = 0xFFu;
constexpr uint32_t FRBS = 272;      // LDS row stride of a 256-byte centroid row (conflict-free b128 column reads)

struct FSmem {
    uint32_t x, ctr, stats;         // shared with the cold layout: the element's packed row, counters, statistics
    uint32_t ppx, red, pp;          // x popcount quarters; fill flags + reduction records; partial intersections (npp x rows x 8 B)
    uint32_t slot0, slot_bytes;     // NS slots of {cent[rows x 272], card[rows], link[rows], rm[rows x 32]}
    uint32_t s_card, s_link, s_rm;  // offsets inside a slot
    uint32_t cold_base;             // where the cold functions' scratch starts (it overlays the LAST slots)
    uint32_t total;
    int ns, npp;
    int cold_slot;                  // first slot the scratch overlaps (ns: none)
};

__host__ __device__ constexpr uint32_t f_align16(size_t v) { return (uint32_t)((v + 15) / 16 * 16); }

__host__ __device__ constexpr FSmem fast_layout(int bf) {
    FSmem f{};
    const size_t rows = (size_t)bf + 1;
    f.x = 0;
    f.ctr = 256;            // 16 u32: counters [0..7], stop reason [8], processed [9]
    f.stats = 256 + 64;     // 8 u64
    f.ppx = 256 + 64 + 64;  // 4 u32
    f.red = f.ppx + 16;     // 2 x 16 B fill flags, then (at +32) TW records of 48 B
    f.pp = f.red + 32 + TW * 48;
    f.npp = 2;  // double-buffered: consecutive compares alternate
    f.slot0 = f_align16(f.pp + (size_t)f.npp * rows * 8);
    f.s_card = f_align16(rows * FRBS);
    f.s_link = f.s_card + f_align16(rows * 4);
    f.s_rm = f.s_link + f_align16(rows * 4);
    f.slot_bytes = f.s_rm + (uint32_t)(rows * 32);
    // scratch of the cold function: the complete engine's layout minus its x / ctr / stats and its one mirror
    // slot (which is slot 0 here)
    const uint32_t cold = smem_layout(bf, 256, 0).total;
    int ns = 8;
    f.cold_slot = 0;
    for (; ns >= 2; --ns) {
        const bool inside = (size_t)(ns - 1) * f.slot_bytes >= cold;  // slot 0 is the cold function's own mirror slot
        const size_t tot = f.slot0 + (size_t)ns * f.slot_bytes + (inside ? 0 : cold);
        if (tot <= 160 * 1024) {
            const int need = (int)((cold + f.slot_bytes - 1) / f.slot_bytes);
            f.cold_slot = inside ? ns - need : ns;
            f.cold_base = f.slot0 + (uint32_t)f.cold_slot * f.slot_bytes;
            f.total = (uint32_t)tot;
            break;
        }
    }
    f.ns = ns;  // 1: does not fit (the host never launches the fast kernel then)
    return f;
}

// the complete engine's LDS layout for its role as the cold function: x / ctr / stats where the fast kernel keeps
// them, one mirror slot (= slot 0, its workspace for splits), everything else from cold_base on
__host__ __device__ constexpr Smem smem_layout_cold(int bf, const FSmem& f) {
    Smem s{};
    SmemCursor c;
    c.off = f.cold_base;
    const int RB = 256;
    const size_t m = (size_t)bf + 1;
    s.x = f.x; s.ctr = f.ctr; s.stats = f.stats;
    s.vec = c.take(RB); s.cA = c.take(RB); s.cB = c.take(RB);
    s.keys = c.take(2 * m * 8); s.link = c.take(2 * m * 4);
    s.i1 = c.take(m * 4); s.u1 = c.take(m * 4); s.i2 = c.take(m * 4); s.u2 = c.take(m * 4);
    s.dst = c.take(m * 4); s.mcard = c.take(m * 4); s.mlink = c.take(m * 4); s.mrm = c.take(m * 32);
    s.red = c.take(2 * TW * NRED * 8);
    s.red32 = c.take(2 * TW * NRED * 4);
    s.wbest = c.take(2 * TW * 8);
    s.path_node = c.take(MAXD * 4); s.path_row = c.take(MAXD * 4); s.path_len = c.take(MAXD * 4);
    s.path_slot = c.take(MAXD * 4); s.path_n = c.take(MAXD * 4);
    s.bc = c.take(16 * 4);
    s.planes = c.take((size_t)TW * NPLW * 64 * 4);
    s.ppart = c.take(2 * (size_t)TW * m * 4);
    s.rc_cent = f.slot0;
    s.rc_card = f.slot0 + f.s_card;
    s.rc_link = f.slot0 + f.s_link;
    s.total = f.total;
    return s;
}

static_assert(fast_layout(50).ns >= 2 && fast_layout(50).total <= 160 * 1024, "bf 50 must fit");
static_assert(fast_layout(254).ns >= 2 && fast_layout(254).total <= 160 * 1024, "bf 254 must fit");

#if defined(__HIPCC__)

// the complete engine as the fast kernel's cold function: compile-time shape, run-time element kind and criterion
template <int BF>
struct KCold : KCBase {
    static constexpr bool dynamic_shape = false;
    static constexpr int F = 2048, nb = 256, RB = 256, RBc = 16, RBS = (int)FRBS;
    static constexpr uint32_t rows = BF + 1, bf = BF, nblk = node_blocks(BF + 1);
    static constexpr int nm = 1;
    static constexpr Smem o = smem_layout_cold(BF, fast_layout(BF));
};

template <int BF>
__device__ __attribute__((noinline)) void cold_insert_one(unsigned char* smem_raw, TreeDev* T, long long e) {
    tree_insert_body<false, KCold<BF>, true>(smem_raw, T, e);
}

// The same context with the one mirror slot pointed at an arbitrary slot of the fast kernel (run-time offsets).
template <int BF>
struct KColdS : KCBase {
    static constexpr bool dynamic_shape = false;
    static constexpr int F = 2048, nb = 256, RB = 256, RBc = 16, RBS = (int)FRBS;
    static constexpr uint32_t rows = BF + 1, bf = BF, nblk = node_blocks(BF + 1);
    static constexpr int nm = 1;
    Smem o;
};

// A leaf that overflowed, split where it lies (_split_node, bitbirch.py:162-211 + update_split_subclusters,
// :289-303), for the common case: the leaf's rows (the appended element included) are in LDS slot `leafsi`, its
// parent P has room for one more row.  The complete engine's split_node works on the slot in place; the parent's two
// rows are rewritten in HBM and - if the parent sits in slot `psi` - in LDS, so that every level above the leaf stays
// valid.  Counters / statistics travel through LDS like in cold_insert_one; ctr[8] returns a stop reason.
template <int BF, bool PROF = false>
__device__ __attribute__((noinline)) void cold_leaf_split(unsigned char* smem_raw, TreeDev* T, long long e, uint32_t nS, uint32_t pcx,
                                                          uint32_t leafnode, uint32_t leafsi, uint32_t P, uint32_t jp, uint32_t lenP,
                                                          uint32_t psi, uint32_t trk) {
    constexpr FSmem f = fast_layout(BF);
    KColdS<BF> k;
    k.cent = T->node_cent; k.card = T->node_card; k.link = T->node_link; k.rm = T->node_rm; k.hdr = T->node_hdr;
    k.scratch = T->scratch_cent; k.cf8 = T->cf8; k.cf16 = T->cf16; k.cf32 = T->cf32;
    k.bufs = T->bufs; k.width = (int)uni((uint32_t)T->width);
    k.crit = 0; k.tol_len = 0; k.thr = 0; k.tolerance = 0; k.tol = nullptr;
    k.L = (LA unsigned char*)smem_raw;
    k.o = smem_layout_cold(BF, f);
    const uint32_t lsb = f.slot0 + leafsi * f.slot_bytes;
    k.o.rc_cent = lsb; k.o.rc_card = lsb + f.s_card; k.o.rc_link = lsb + f.s_link;
    const int tid = threadIdx.x;
    LA uint32_t* lctr = (LA uint32_t*)(k.L + f.ctr);
    LA uint32_t* bc = lds<uint32_t>(k.L, k.o.bc);
    Elem el;
    el.idx = e; el.nS = nS; el.s1S = 0; el.s2S = 0; el.pcx = pcx;
    __syncthreads();
    uint32_t cN = uni(lctr[C_NODES]), c32 = uni(lctr[C_N32]), cFirst = uni(lctr[C_FIRST_LEAF]);
    int red_slot = 0, cmp_par = 0;
    u64 sph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    split_node<false, PROF>(k, el, red_slot, cmp_par, leafnode, 0u, true, trk, cN, c32, cFirst, T->ctr, sph);
    if constexpr (PROF) {
        if (tid == 0)
            for (int i = 0; i < 8; ++i) T->sphase[i] += sph[i];
    }
    const uint32_t node1 = uni(bc[0]), cardA = uni(bc[3]), cardB = uni(bc[4]);
    const uint32_t nA = uni(bc[7]), nB = uni(bc[8]);
    const uint32_t slotA = (2u << 30) | uni(bc[9]), slotB = (2u << 30) | uni(bc[10]);
    const uint32_t bad = uni(bc[11]);
    // update_split_subclusters (bitbirch.py:289-303): row jp now tracks node1, a new row tracks the split node
    node_put_row(k, P, jp, k.o.cA, cardA, node1, NONE, nA, slotA, 0, 0);
    node_put_row(k, P, lenP, k.o.cB, cardB, leafnode, NONE, nB, slotB, 0, 0);
    if (psi != F_NOSLOT) {
        const uint32_t pb = f.slot0 + psi * f.slot_bytes;
        if (tid < 16) {
            *(LA u32x4_t*)(k.L + pb + jp * FRBS + tid * 16) = lds<u32x4_t>(k.L, k.o.cA)[tid];
            *(LA u32x4_t*)(k.L + pb + lenP * FRBS + tid * 16) = lds<u32x4_t>(k.L, k.o.cB)[tid];
        }
        if (tid == 64) {
            u32x4_t a;
            a.x = NONE; a.y = nA; a.z = slotA; a.w = 0;
            *(LA u32x4_t*)(k.L + pb + f.s_rm + jp * 32) = a;
            *(LA u32x4_t*)(k.L + pb + f.s_rm + jp * 32 + 16) = (u32x4_t)(0);
            a.y = nB; a.z = slotB;
            *(LA u32x4_t*)(k.L + pb + f.s_rm + lenP * 32) = a;
            *(LA u32x4_t*)(k.L + pb + f.s_rm + lenP * 32 + 16) = (u32x4_t)(0);
            *(LA uint32_t*)(k.L + pb + f.s_card + jp * 4) = cardA;
            *(LA uint32_t*)(k.L + pb + f.s_card + lenP * 4) = cardB;
            *(LA uint32_t*)(k.L + pb + f.s_link + jp * 4) = node1;
            *(LA uint32_t*)(k.L + pb + f.s_link + lenP * 4) = leafnode;
        }
    }
    if (tid == 0) {
        stg<uint32_t>(k.hdr + P, lenP + 1);
        lctr[C_NODES] = cN; lctr[C_N32] = c32; lctr[C_FIRST_LEAF] = cFirst;
        lctr[8] = bad ? (uint32_t)STOP_RANGE : (uint32_t)STOP_DONE;
    }
    __syncthreads();
}

// wave-uniform value parked in a VGPR: the compiler cannot prove it uniform, so it stays out of the scalar file
__device__ __forceinline__ uint32_t vpark(uint32_t v) {
    uint32_t r = v;
    asm("" : "+v"(r));  // (no instruction of its own: the value is made a VGPR the optimiser cannot see through)
    return r;
}

// the thread index as a value the optimiser cannot see through: predicates built from it (tid < 16, lane == 63 ...)
// are recomputed where they are used (one v_cmp) instead of being hoisted out of the insertion loop into scalar
// register pairs, of which there are not enough (they came back as v_readlane spill reloads)
__device__ __forceinline__ int ftid() {
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

__device__ __forceinline__ u64 vpark64(u64 v) {
    return ((u64)vpark((uint32_t)(v >> 32)) << 32) | vpark((uint32_t)v);
}

// DPP steps written so that the compiler folds each into ONE v_max_u32_dpp / v_add_u32_dpp: `old` is the
// operation's identity (0 for unsigned max and for add), which is what lanes of masked-out rows must keep
template <int N>
__device__ __forceinline__ uint32_t ror_any(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 + N, 0xF, 0xF, false);
}
template <unsigned CTRL, unsigned ROWMASK>
__device__ __forceinline__ uint32_t bcast0(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xF, false);
}
// maximum / sum over the wave, valid in lane 63
__device__ __forceinline__ uint32_t wave_max63(uint32_t v) {
    uint32_t o;
    o = ror_any<8>(v); v = o > v ? o : v;
    o = ror_any<4>(v); v = o > v ? o : v;
    o = ror_any<2>(v); v = o > v ? o : v;
    o = ror_any<1>(v); v = o > v ? o : v;
    o = bcast0<0x142, 0xA>(v); v = o > v ? o : v;  // row_bcast15: rows 1 and 3 also see rows 0 and 2
    o = bcast0<0x143, 0xC>(v); v = o > v ? o : v;  // row_bcast31: rows 2 and 3 also see rows 0 and 1
    return v;
}
__device__ __forceinline__ uint32_t wave_min63(uint32_t v) { return ~wave_max63(~v); }
__device__ __forceinline__ uint32_t wave_sum63(uint32_t v) {
    v += ror_any<8>(v);
    v += ror_any<4>(v);
    v += ror_any<2>(v);
    v += ror_any<1>(v);
    v += bcast0<0x142, 0xA>(v);
    v += bcast0<0x143, 0xC>(v);
    return v;
}
__device__ __forceinline__ u64 wave_sum63_64(u64 v) {
    v += ror64<8>(v);
    v += ror64<4>(v);
    v += ror64<2>(v);
    v += ror64<1>(v);
    v += ((u64)bcast0<0x142, 0xA>((uint32_t)(v >> 32)) << 32) | bcast0<0x142, 0xA>((uint32_t)v);
    v += ((u64)bcast0<0x143, 0xC>((uint32_t)(v >> 32)) << 32) | bcast0<0x143, 0xC>((uint32_t)v);
    return v;
}

#define F_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// Order-exact key of the similarity inter / max(union, 1) (similarity.cpp:326-331) for unions <= 4096: the bit
// pattern of the correctly rounded float32 quotient.  See the header of this file.
__device__ __forceinline__ uint32_t sim_key(uint32_t inter, uint32_t un) {
    return __float_as_uint(__fdiv_rn((float)inter, (float)un));
}

struct KFCtx : KCBase {
    static constexpr int F = 2048, nb = 256, RB = 256;
};

// linear-sum values of BitFeature buffer row `e` for features b*8 .. b*8+7 (the buffer branch of elem_cols)
__device__ __forceinline__ void buf_cols(const uint8_t* bufs, int width, long long e, int b, uint32_t v[8]) {
    const size_t base = (size_t)e * 2049 + (size_t)b * 8;
    if (width == 1) {
        const u32x2_t q = ldg<u32x2_t>(bufs + base);
        v[0] = q.x & 0xFF; v[1] = (q.x >> 8) & 0xFF; v[2] = (q.x >> 16) & 0xFF; v[3] = q.x >> 24;
        v[4] = q.y & 0xFF; v[5] = (q.y >> 8) & 0xFF; v[6] = (q.y >> 16) & 0xFF; v[7] = q.y >> 24;
    } else if (width == 2) {
        const u32x4_t q = ldg<u32x4_t>(bufs + 2 * base);
        v[0] = q.x & 0xFFFF; v[1] = q.x >> 16; v[2] = q.y & 0xFFFF; v[3] = q.y >> 16;
        v[4] = q.z & 0xFFFF; v[5] = q.z >> 16; v[6] = q.w & 0xFFFF; v[7] = q.w >> 16;
    } else if (width == 4) {
        const u32x4_t q0 = ldg<u32x4_t>(bufs + 4 * base), q1 = ldg<u32x4_t>(bufs + 4 * base + 16);
        v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w;
        v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
    } else {
#pragma unroll
        for (int q = 0; q < 8; q += 2) {  // uint64 tables: values fit 32 bits by contract (n_samples < 2^32)
            const u32x4_t w = ldg<u32x4_t>(bufs + 8 * (base + q));
            v[q] = w.x;
            v[q + 1] = w.z;
        }
    }
}

struct FLevels {  // per level of the path, wave-uniform, parked in VGPRs
    uint32_t tag[FMAXLV], len[FMAXLV], fl[FMAXLV];     // node id (NONE: invalid); rows; F_LEAF | F_ZERO | slot << 8 (F_NOSLOT: tag only)
    uint32_t link0[FMAXLV], ts0[FMAXLV], tn0[FMAXLV];  // tag-only (all-zero) levels: row 0's child, tracking CF slot, n_samples
};

template <int BFv, int BUFv, int CRITv>
struct KF {
    static constexpr int BF = BFv, BUF = BUFv, CRIT = CRITv;
    static constexpr uint32_t rows = BFv + 1, bf = BFv, nblk = node_blocks(BFv + 1);
    static constexpr int passes = (BFv + 1 + 63) / 64;
    static constexpr FSmem f = fast_layout(BFv);
};

// ---- fill slot `si` with node `nd` (one memory round trip; one barrier) ------------------------------------
// Returns through `lv` the level record.  All rows of the node are requested without waiting for its length;
// a node without any non-zero centroid among its rows keeps only a tag.
template <int Q, class K>
__device__ __forceinline__ void fast_fill(const KCBase& k, LA unsigned char* L, uint32_t nd, uint32_t si, FLevels& lv, int& bpar) {
    constexpr FSmem f = K::f;
    constexpr uint32_t rows = K::rows;
    const int tid = ftid();
    const size_t meta = (size_t)nd * NG;
    // (only {length, leaf word} of the 16-byte header: with a 16-byte load the two dead registers of its destination were
    // reused as address scratch at once - a write-after-write hazard the compiler resolved with s_waitcnt vmcnt(0) right
    // behind the load, i.e. the fill made TWO memory round trips, header first)
    const u32x2_t hraw = ldg<u32x2_t>(k.hdr + nd);
    constexpr int NCH = (int)((rows * 16 + TB - 1) / TB);  // 16-byte centroid pieces per thread
    u32x4_t c[NCH];
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
        const uint32_t i = (uint32_t)u * TB + tid;
        c[u] = ldg<u32x4_t>(k.cent + (meta * 16 + (i < rows * 16 ? i : rows * 16 - 1)) * 16);
    }
    constexpr int NRM = (int)((rows * 2 + TB - 1) / TB);  // 16-byte RowMeta pieces per thread
    u32x4_t m[NRM];
#pragma unroll
    for (int u = 0; u < NRM; ++u) {
        const uint32_t i = (uint32_t)u * TB + tid;
        m[u] = ldg<u32x4_t>((const uint8_t*)(k.rm + meta) + (size_t)(i < rows * 2 ? i : rows * 2 - 1) * 16);
    }
    const uint32_t rcl = (uint32_t)tid < rows ? tid : rows - 1;
    const uint32_t cd = ldg<uint32_t>(k.card + meta + rcl);
    const uint32_t lk = ldg<uint32_t>(k.link + meta + rcl);
    // a sealed node (capacity below bf + 1, bb_tree.hip "Node storage") is nothing this kernel inserts into: it reports
    // length 0, which sends the element to the complete engine (that thaws the node) like the first element of a tree
    const bool sealed = hw_cap(uni(hraw.y)) < rows;
    const uint32_t len = sealed ? 0u : uni(hraw.x), leaf = uni(hraw.y) & HW_LEAF;
    const uint32_t sbase = f.slot0 + __umul24(si, f.slot_bytes);
    // (every loaded register is consumed on every path - threads beyond the node's last piece re-write that piece, whose
    // index their load was clamped to: a load whose only use sits behind a branch stays "pending" for the compiler on
    // the path around it, and every later reuse of its destination register then waits with vmcnt(0), i.e. for the
    // tracking-CF loads that are meant to stay in flight across the deeper levels)
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
        const uint32_t i0 = (uint32_t)u * TB + tid;
        const uint32_t i = i0 < rows * 16 ? i0 : rows * 16 - 1;
        *(LA u32x4_t*)(L + sbase + (i >> 4) * FRBS + (i & 15) * 16) = c[u];
    }
#pragma unroll
    for (int u = 0; u < NRM; ++u) {
        const uint32_t i0 = (uint32_t)u * TB + tid;
        const uint32_t i = i0 < rows * 2 ? i0 : rows * 2 - 1;
        *(LA u32x4_t*)(L + sbase + f.s_rm + i * 16) = m[u];
    }
    *(LA uint32_t*)(L + sbase + f.s_card + rcl * 4) = cd;
    *(LA uint32_t*)(L + sbase + f.s_link + rcl * 4) = lk;
    // any non-zero centroid among the node's rows?  (block-wide OR through the reduction scratch)
    const bool nz = (uint32_t)tid < len && cd != 0;
    bpar ^= 1;
    const u64 bal = __ballot(nz);
    LA uint32_t* anyw = (LA uint32_t*)(L + f.red) + bpar * 4;
    if ((tid & 63) == 0) anyw[tid >> 6] = bal != 0ull ? 1u : 0u;
    F_LDS_BARRIER();
    const u32x4_t a4 = *(LA u32x4_t*)(L + f.red + bpar * 16);
    const bool any = uni(a4.x | a4.y | a4.z | a4.w) != 0;
    // row 0's data matter for tag-only levels only (where every element goes: all similarities are 0)
    const u32x4_t r0 = *(LA u32x4_t*)(L + sbase + f.s_rm);
    const uint32_t l0 = *(LA uint32_t*)(L + sbase + f.s_link);
    const bool tagonly = !any && !leaf;
    lv.tag[Q] = vpark(sealed ? NONE : nd);
    lv.len[Q] = vpark(len);
    lv.fl[Q] = vpark(tagonly ? (F_ZERO | (F_NOSLOT << 8)) : ((leaf ? F_LEAF : 0u) | (si << 8)));
    lv.link0[Q] = vpark(l0);
    lv.ts0[Q] = vpark(r0.z);
    lv.tn0[Q] = vpark(r0.y);
}

// compile-time loop: fn(std::integral_constant<int, I>) for I in [I0, N) - every index below is a constant, so the
// per-level arrays are registers, never scratch memory (a `#pragma unroll` the compiler declines would put them there)
template <int I, int N, class Fn>
__device__ __forceinline__ void static_for(Fn&& fn) {
    if constexpr (I < N) {
        fn(std::integral_constant<int, I>{});
        static_for<I + 1, N>(fn);
    }
}

// the row a node compare chose, with everything the insertion needs about it (wave-uniform)
struct FRow {
    uint32_t j, link;
    u32x4_t a, b;  // RowMeta image: {BitFeature id, n_samples, CF slot, -} {sum(ls) lo/hi, sum(ls^2) lo/hi}
};

// popcount of a 16-byte piece added to `acc`: v_bcnt_u32_b32 accumulates for free, but the compiler re-associates the
// sums of a row into a tree of separate adds (no use to a wave that issues alone)
__device__ __forceinline__ uint32_t popc4v_acc(u32x4_t q, uint32_t acc) {
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(q.x));
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(q.y));
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(q.z));
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(q.w));
    return acc;
}

// ---- first-argmax of the similarity of x to the rows of the node in slot `si` (one LDS barrier) -----------
// Phase 1: every lane ANDs + popcounts this wave's quarter of "its" row; the partial intersections meet in LDS.
// Phase 2 (every wave redundantly): row similarity key, wave maximum, first lane holding it.  The row's link and
// RowMeta are read by every lane for its own row together with the popcount, so that the winner's come out of a
// v_readlane instead of another LDS round trip (nodes of up to 64 rows).
// phase 1 into partial buffer `pb`
template <class K>
__device__ __forceinline__ void compare_phase1(LA unsigned char* L, uint32_t si, uint32_t len, const u32x4_t (&xv)[4], uint32_t pcx,
                                               uint32_t pb) {
    constexpr FSmem f = K::f;
    constexpr uint32_t rows = K::rows;
    const int tid = ftid(), wave = tid >> 6, lane = tid & 63;
    const uint32_t sbase = f.slot0 + __umul24(si, f.slot_bytes);
    const uint32_t last = len - 1;  // len >= 1
    if constexpr (K::passes > 1) {
        // Nodes of up to 256 rows (bf 254): wave w owns rows 64 w .. 64 w + 63, one WHOLE row per lane against the
        // element's row in LDS (f.x: broadcast reads) - no partial intersections to exchange, the similarity key once
        // per row instead of once per wave and row.  Each wave publishes its first-argmax with the row's link and
        // RowMeta; phase 2 picks among the four.
        static_assert(K::rows <= 64 * TW, "one row per lane");
        const uint32_t r = (uint32_t)wave * 64 + lane;
        const uint32_t rc = r < last ? r : last;
        const uint32_t base = sbase + rc * FRBS;
        uint32_t inter = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const u32x4_t d = *(LA u32x4_t*)(L + base + i * 16);
            const u32x4_t xq = *(LA u32x4_t*)(L + f.x + i * 16);
            inter = popc4v_acc(d & xq, inter);
        }
        const uint32_t card = *(LA uint32_t*)(L + sbase + f.s_card + rc * 4);
        const uint32_t lk = *(LA uint32_t*)(L + sbase + f.s_link + rc * 4);
        const u32x4_t ma = *(LA u32x4_t*)(L + sbase + f.s_rm + rc * 32);
        const u32x4_t mb = *(LA u32x4_t*)(L + sbase + f.s_rm + rc * 32 + 16);
        uint32_t un = card + pcx - inter;
        un = un < 1u ? 1u : un;
        const uint32_t key = r < len ? sim_key(inter, un) : 0u;
        const uint32_t kmax = rdlane(wave_max63(key), 63);
        const u64 m = __ballot(r < len && key == kmax);
        const bool valid = m != 0ull;  // (a wave whose rows all lie beyond the node's length has no candidate)
        const int j = valid ? __ffsll((long long)m) - 1 : 0;
        u32x4_t c0, c1, c2;
        c0.x = kmax; c0.y = valid ? (uint32_t)wave * 64 + (uint32_t)j : 0xFFFFu; c0.z = rdlane(lk, j); c0.w = 0;
        c1.x = rdlane(ma.x, j); c1.y = rdlane(ma.y, j); c1.z = rdlane(ma.z, j); c1.w = 0;
        c2.x = rdlane(mb.x, j); c2.y = rdlane(mb.y, j); c2.z = rdlane(mb.z, j); c2.w = rdlane(mb.w, j);
        if (lane == 0) {
            LA unsigned char* cand = L + f.pp + (pb * TW + (uint32_t)wave) * 64;  // the partial buffers' space: 2 x 4 records
            *(LA u32x4_t*)(cand) = c0;
            *(LA u32x4_t*)(cand + 16) = c1;
            *(LA u32x4_t*)(cand + 32) = c2;
        }
        return;
    }
    LA uint16_t* pp = (LA uint16_t*)(L + f.pp + pb * rows * 8);
#pragma unroll
    for (int p = 0; p < K::passes; ++p) {
        const uint32_t r = (uint32_t)p * 64 + lane;
        const uint32_t rc = r < last ? r : last;
        const uint32_t base = sbase + rc * FRBS + (uint32_t)wave * 64;
        u32x4_t d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = *(LA u32x4_t*)(L + base + i * 16);
        uint32_t part = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) part = popc4v_acc(d[i] & xv[i], part);
        if (r < rows) pp[r * 4 + wave] = (uint16_t)part;
    }
}

// phase 2 from partial buffer `pb` (behind a barrier that follows phase 1)
template <class K>
__device__ __forceinline__ void compare_phase2(LA unsigned char* L, uint32_t si, uint32_t len, bool leaf, uint32_t pcx, uint32_t pb, FRow& out) {
    constexpr FSmem f = K::f;
    constexpr uint32_t rows = K::rows;
    const int lane = ftid() & 63;
    const uint32_t sbase = f.slot0 + __umul24(si, f.slot_bytes);
    LA uint16_t* pp = (LA uint16_t*)(L + f.pp + pb * rows * 8);
    const uint32_t last = len - 1;
    if constexpr (K::passes == 1) {
        const uint32_t r = lane;
        const uint32_t rc = r < last ? r : last;
        const u32x2_t q = *(LA u32x2_t*)(pp + rc * 4);
        const uint32_t card = *(LA uint32_t*)(L + sbase + f.s_card + rc * 4);
        const uint32_t lk = *(LA uint32_t*)(L + sbase + f.s_link + rc * 4);
        const u32x4_t ma = *(LA u32x4_t*)(L + sbase + f.s_rm + rc * 32);
        u32x4_t mb = (u32x4_t)(0);
        if (leaf) mb = *(LA u32x4_t*)(L + sbase + f.s_rm + rc * 32 + 16);
        const uint32_t inter = (q.x & 0xFFFFu) + (q.x >> 16) + (q.y & 0xFFFFu) + (q.y >> 16);
        uint32_t un = card + pcx - inter;
        un = un < 1u ? 1u : un;
        const uint32_t key = r < len ? sim_key(inter, un) : 0u;
        const uint32_t kmax = rdlane(wave_max63(key), 63);
        const u64 m = __ballot(r < len && key == kmax);
        const int j = __ffsll((long long)m) - 1;
        out.j = (uint32_t)j;
        out.link = rdlane(lk, j);
        out.a.x = rdlane(ma.x, j); out.a.y = rdlane(ma.y, j); out.a.z = rdlane(ma.z, j); out.a.w = 0;
        if (leaf) { out.b.x = rdlane(mb.x, j); out.b.y = rdlane(mb.y, j); out.b.z = rdlane(mb.z, j); out.b.w = rdlane(mb.w, j); }
        else out.b = (u32x4_t)(0);
    } else {
        // the four waves' candidates (phase 1): highest key, lowest row among equals - waves hold ascending rows
        const LA unsigned char* cand = L + f.pp + pb * TW * 64;
        uint32_t bw = 0;
        uint32_t bkey = uni(*(const LA uint32_t*)(cand));  // wave 0 always has a candidate: len >= 1
#pragma unroll
        for (int w = 1; w < TW; ++w) {
            const u32x2_t kr = *(const LA u32x2_t*)(cand + w * 64);
            const uint32_t kw = uni(kr.x), rw = uni(kr.y);
            const bool take = rw != 0xFFFFu && kw > bkey;
            bkey = take ? kw : bkey;
            bw = take ? (uint32_t)w : bw;
        }
        const u32x4_t c0 = *(const LA u32x4_t*)(cand + bw * 64);
        const u32x4_t c1 = *(const LA u32x4_t*)(cand + bw * 64 + 16);
        const u32x4_t c2 = *(const LA u32x4_t*)(cand + bw * 64 + 32);
        out.j = uni(c0.y);
        out.link = uni(c0.z);
        out.a.x = uni(c1.x); out.a.y = uni(c1.y); out.a.z = uni(c1.z); out.a.w = 0;
        out.b.x = uni(c2.x); out.b.y = uni(c2.y); out.b.z = uni(c2.z); out.b.w = uni(c2.w);
    }
}

// fn(level) for the tracking levels 0 .. D-1 of the path, nested: ONE taken branch (at level D) instead of one per
// level beyond D - a wave that runs alone on its SIMD pays an instruction refetch for every taken branch
template <int Q, class Fn>
__device__ __forceinline__ void for_levels(int D, Fn&& fn) {
    if constexpr (Q < FMAXT) {
        if (Q < D) {
            fn(std::integral_constant<int, Q>{});
            for_levels<Q + 1>(D, fn);
        }
    }
}

struct FProf {  // shader-clock cycles per phase (PROF builds only)
    u64 ph[16];
    u64 mark;
};
template <bool PROF>
__device__ __forceinline__ void fprof(FProf& pr, int i) {
    if constexpr (PROF) {
        const u64 n = __builtin_amdgcn_s_memtime();
        pr.ph[i] += n - pr.mark;
        pr.mark = n;
    }
}

struct FPath {  // the root-to-leaf path of the element being inserted (wave-uniform)
    uint32_t nd;
    int D;      // leaf level, -1 while descending
    bool cold;  // this element needs the complete engine
    uint32_t leaflen, leafsi, leafnode, ns_above, calls, rows_cmp;
    FRow leaf;  // the chosen leaf row
    uint32_t p_node[FMAXT], p_row[FMAXT], p_ts[FMAXT], p_tn[FMAXT], p_si[FMAXT];
};

// Tracking cluster features (cf32 rows of 2048 features, 8 per thread) of the current path, one per level, kept in
// REGISTERS across insertions and written back only when a level's tracking row changes: the upper levels of a tree
// keep routing to the same row for long runs, so their 8 KB read-modify-write per insertion disappears.  HBM is
// stale for the cached rows until they are evicted or flushed (fast_run flushes before it returns, i.e. before any
// code that reads tracking CFs from HBM can run).
struct FCfCache {
    uint32_t tag[FMAXT];     // cf32 slot index held for the level (NONE: nothing), parked
    uint32_t v[FMAXT][8];
};

template <int Q>
__device__ __forceinline__ void cf_cache_put(const KFCtx& k, const FCfCache& C) {
    const size_t idx = (size_t)uni(C.tag[Q]) * 2048 + (size_t)threadIdx.x * 8;
    u32x4_t q0, q1;
    q0.x = C.v[Q][0]; q0.y = C.v[Q][1]; q0.z = C.v[Q][2]; q0.w = C.v[Q][3];
    q1.x = C.v[Q][4]; q1.y = C.v[Q][5]; q1.z = C.v[Q][6]; q1.w = C.v[Q][7];
    stg<u32x4_t>(k.cf32 + idx, q0);
    stg<u32x4_t>(k.cf32 + idx + 4, q1);
}

// make level Q's cache hold cf32 slot `ts` (requested here, consumed after the descent)
template <int Q>
__device__ __forceinline__ void cf_cache_want(const KFCtx& k, FCfCache& C, uint32_t ts) {
    const uint32_t want = ts & 0x3FFFFFFFu;
    const uint32_t have = uni(C.tag[Q]);
    if (have == want) return;
    if (have != NONE) cf_cache_put<Q>(k, C);
    const size_t idx = (size_t)want * 2048 + (size_t)threadIdx.x * 8;
    const u32x4_t q0 = ldg<u32x4_t>(k.cf32 + idx), q1 = ldg<u32x4_t>(k.cf32 + idx + 4);
    C.v[Q][0] = q0.x; C.v[Q][1] = q0.y; C.v[Q][2] = q0.z; C.v[Q][3] = q0.w;
    C.v[Q][4] = q1.x; C.v[Q][5] = q1.y; C.v[Q][6] = q1.z; C.v[Q][7] = q1.w;
    C.tag[Q] = vpark(want);
}

// one level of the greedy descent (bitbirch.py:305-357), then the next
template <int Q, class K, bool PROF>
__device__ __forceinline__ void fast_level(const KFCtx& k, LA unsigned char* L, FLevels& lv, FPath& P, FCfCache& C,
                                           const u32x4_t (&xv)[4], uint32_t pcx, int& cpar, int& bpar, FProf& pr) {
    constexpr FSmem f = K::f;
    constexpr int NS = f.ns;
    const uint32_t nd = P.nd;
    const uint32_t want_si = P.ns_above < (uint32_t)(NS - 1) ? P.ns_above : (uint32_t)(NS - 1);
    bool hit = uni(lv.tag[Q]) == nd;
    if (hit) {
        const uint32_t fl0 = uni(lv.fl[Q]);
        if ((fl0 >> 8) != F_NOSLOT && (fl0 >> 8) != want_si) hit = false;
    }
    if (!hit) {
        // whoever holds the slot loses it
        static_for<0, FMAXLV>([&](auto z) {
            if constexpr (z.value != Q) {
                if ((uni(lv.fl[z.value]) >> 8) == want_si) {
                    lv.tag[z.value] = vpark(NONE);
                    // a level ABOVE on this very path (the last slot is shared by all deep levels): its update at
                    // the end of the insertion must not write into the slot any more
                    if constexpr (z.value < Q && z.value < FMAXT) P.p_si[z.value] = vpark(F_NOSLOT);
                }
            }
        });
        fast_fill<Q, K>(k, L, nd, want_si, lv, bpar);  // (ends with a barrier: the slot is complete)
        fprof<PROF>(pr, 8);  // [8] fills, [11] their count
        if constexpr (PROF) pr.ph[11] += 1;
    }
    const uint32_t fl = uni(lv.fl[Q]), len = uni(lv.len[Q]);
    if (len == 0) {  // an empty root: the first element of the tree
        P.cold = true;
        return;
    }
    P.calls += 1;
    P.rows_cmp += len;
    const uint32_t si = fl >> 8;
    FRow row;
    if (fl & F_ZERO) {
        row.j = 0;
        row.link = uni(lv.link0[Q]);
        row.a.x = NONE; row.a.y = uni(lv.tn0[Q]); row.a.z = uni(lv.ts0[Q]); row.a.w = 0;
        row.b = (u32x4_t)(0);
        fprof<PROF>(pr, 9);  // [9] tag-only levels, [12] count
        if constexpr (PROF) pr.ph[12] += 1;
    } else {
        cpar ^= 1;
        compare_phase1<K>(L, si, len, xv, pcx, (uint32_t)cpar);
        F_LDS_BARRIER();
        compare_phase2<K>(L, si, len, (fl & F_LEAF) != 0, pcx, (uint32_t)cpar, row);
        P.ns_above += 1;
        fprof<PROF>(pr, 10);  // [10] compares, [13] count
        if constexpr (PROF) pr.ph[13] += 1;
    }
    if (fl & F_LEAF) {
        P.D = Q;
        P.leaf.j = row.j; P.leaf.link = row.link;
        P.leaf.a.x = vpark(row.a.x); P.leaf.a.y = vpark(row.a.y); P.leaf.a.z = vpark(row.a.z); P.leaf.a.w = 0;
        P.leaf.b.x = vpark(row.b.x); P.leaf.b.y = vpark(row.b.y); P.leaf.b.z = vpark(row.b.z); P.leaf.b.w = vpark(row.b.w);
        P.leaflen = len; P.leafsi = si; P.leafnode = nd;
        return;
    }
    if constexpr (Q + 1 < FMAXLV) {
        // (only ever operands of per-lane arithmetic from here on: parked in VGPRs, out of the scalar file)
        P.p_node[Q] = vpark(nd); P.p_row[Q] = vpark(row.j); P.p_ts[Q] = vpark(row.a.z); P.p_tn[Q] = vpark(row.a.y);
        P.p_si[Q] = vpark((fl & F_ZERO) ? F_NOSLOT : si);
        cf_cache_want<Q>(k, C, row.a.z);  // the tracking CF is on its way while the deeper levels are compared
        P.nd = row.link;
        fast_level<Q + 1, K, PROF>(k, L, lv, P, C, xv, pcx, cpar, bpar, pr);
    } else {
        P.cold = true;  // deeper than this kernel's path registers
    }
}

// ---- the steady-state loop ---------------------------------------------------------------------------------
// Inserts elements e0, e0+1, ... until one needs the complete engine: returns that element's index with nothing of
// it applied (or n_elems when the batch is done / a pool ran full - the stop reason is in ctr[8]).  Free of calls and
// with no state of its own that outlives it, so that nothing but three scalars is live across the call of the cold
// function in the caller: counters and statistics travel through LDS (f.ctr / f.stats); the slots start empty at
// every entry (the cold function that ran in between used them as scratch).
template <class K, bool PROF>
__device__ __forceinline__ long long fast_run(unsigned char* smem_raw, TreeDev* T, long long e0, bool resume) {
    constexpr FSmem f = K::f;
    constexpr uint32_t bf = K::bf;
    constexpr int F = 2048;
    KFCtx k;
    // pool pointers are wave-uniform but only ever feed per-lane address arithmetic: parked in VGPRs
    k.cent = (uint8_t*)vpark64((u64)(uintptr_t)T->node_cent); k.card = (uint32_t*)vpark64((u64)(uintptr_t)T->node_card);
    k.link = (uint32_t*)vpark64((u64)(uintptr_t)T->node_link); k.rm = (RowMeta*)vpark64((u64)(uintptr_t)T->node_rm);
    k.hdr = (NodeHdr*)vpark64((u64)(uintptr_t)T->node_hdr);
    k.scratch = nullptr; k.cf8 = (uint8_t*)vpark64((u64)(uintptr_t)T->cf8); k.cf16 = (uint16_t*)vpark64((u64)(uintptr_t)T->cf16);
    k.cf32 = (uint32_t*)vpark64((u64)(uintptr_t)T->cf32);
    k.bufs = (const uint8_t*)vpark64((u64)(uintptr_t)T->bufs); k.width = (int)uni((uint32_t)T->width);
    k.crit = (int)uni((uint32_t)T->crit); k.tol_len = (int)uni((uint32_t)T->tol_len); k.thr = T->thr; k.tolerance = T->tolerance;
    k.tol = T->tol_table;
    LA unsigned char* L = (LA unsigned char*)smem_raw;
    k.L = L;
    const int tid0 = threadIdx.x;
    const uint8_t* in_rows = (const uint8_t*)vpark64((u64)(uintptr_t)T->rows);
    // (loaded through a pointer the compiler does not know to be uniform: made scalar values by hand, so that the loop
    // counter, its compares and the row address of the prefetch are scalar arithmetic)
    const long long row_stride = T->row_stride;
    const long long n_elems = T->n_elems;
    uint32_t* out_leaf = (uint32_t*)vpark64((u64)(uintptr_t)T->out_leaf);
    const bool have_out = T->out_leaf != nullptr;
    const uint32_t cap8 = uni(T->cap8);
    constexpr bool bufmode = K::BUF == 1;
    const int crit = K::CRIT >= 0 ? K::CRIT : k.crit;
    LA uint32_t* lctr = (LA uint32_t*)(L + f.ctr);
    LA u64* lstats = (LA u64*)(L + f.stats);
    // counters the fast path changes (wave-uniform registers); the others stay in LDS for the cold function
    uint32_t cI = uni(lctr[C_IDS]), c8 = uni(lctr[C_N8]);
    const uint32_t cRoot = uni(lctr[C_ROOT]);
    uint32_t st_calls = 0, st_rows = 0, st_merge = 0, st_append = 0, st_depth = 0;  // statistics since the last flush
    FLevels lv;
    {
        // after an in-place leaf split (which runs OUTSIDE this function, see tree_fast_body) the level records come
        // back from LDS: the slots above the split leaf are still valid
        LA uint32_t* stash = (LA uint32_t*)(L + f.pp);
        static_for<0, FMAXLV>([&](auto q) {
            constexpr int z = q.value;
            const u32x4_t a = *(LA u32x4_t*)(stash + z * 8);
            const u32x2_t b = *(LA u32x2_t*)(stash + z * 8 + 4);
            lv.tag[z] = vpark(resume ? uni(a.x) : NONE); lv.len[z] = vpark(resume ? uni(a.y) : 0u); lv.fl[z] = vpark(resume ? uni(a.z) : 0u);
            lv.link0[z] = vpark(resume ? uni(a.w) : 0u); lv.ts0[z] = vpark(resume ? uni(b.x) : 0u); lv.tn0[z] = vpark(resume ? uni(b.y) : 0u);
        });
        __syncthreads();  // (the compares' partial buffers share the stash's space)
    }
    FCfCache C;
    static_for<0, FMAXT>([&](auto q) {
        C.tag[q.value] = vpark(NONE);
        static_for<0, 8>([&](auto z) { C.v[q.value][z.value] = 0; });
    });
    int cpar = 0, bpar = 0;
    FProf pr;
    static_for<0, 16>([&](auto i) { pr.ph[i.value] = 0; });
    pr.mark = PROF ? __builtin_amdgcn_s_memtime() : 0;
#define FPH(i) fprof<PROF>(pr, i)

    // packed fingerprints: what a thread needs of the NEXT row is requested one insertion ahead, straight into
    // registers (the host only launches this kernel on 16-byte aligned rows): this wave's quarter of the row (the
    // same 64 bytes in every lane), the thread's own byte (its 8 features), one dword per lane for the popcount
    u32x4_t nq[4] = {(u32x4_t)(0), (u32x4_t)(0), (u32x4_t)(0), (u32x4_t)(0)};
    uint32_t nb = 0, nw = 0;
    // (branch-free: the row index is clamped, never predicated - a conditional request would make the compiler
    // copy the loaded registers at the end of the branch, i.e. wait for the loads it has just issued)
    auto prefetch = [&](long long ee) {
        const int tid = tid0, wave = tid >> 6, lane = tid & 63;
        const long long ec = ee < n_elems ? ee : n_elems - 1;
        const uint8_t* row = in_rows + (size_t)ec * (size_t)row_stride;
#pragma unroll
        for (int i = 0; i < 4; ++i) nq[i] = ldg<u32x4_t>(row + (uint32_t)wave * 64 + i * 16);
        nb = ldg<uint8_t>(row + tid);
        nw = ldg<uint32_t>(row + lane * 4);
    };
    // ... and consumed (moved into the "current element" registers below) BEFORE the insertion in progress issues its
    // stores: on gfx9-family ISAs loads and stores share vmcnt and complete out of order with respect to each other,
    // so waiting for a load with stores in flight means waiting for all of them.
    u32x4_t cxv[4] = {(u32x4_t)(0), (u32x4_t)(0), (u32x4_t)(0), (u32x4_t)(0)};
    uint32_t cxb = 0, cpc = 0;
    auto take_prefetched = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) cxv[i] = nq[i];
        cxb = nb;
        cpc = rdlane(wave_sum63((uint32_t)__popc(nw)), 63);
    };
    if constexpr (!bufmode) {
        if (e0 < n_elems) {
            prefetch(e0);
            take_prefetched();
            prefetch(e0 + 1);
        }
    }

    long long e = e0;
    int stop = STOP_DONE;
    bool cold = false, split_exit = false;
    while (e < n_elems) {
        const int tid = ftid(), wave = tid >> 6, lane = tid & 63;
        // ---- the element: packed centroid, popcount (and, for BitFeature buffers, n and the moments) --------------
        uint32_t nS = 1;
        u64 s1S = 0, s2S = 0;
        uint32_t xs[8], xb;
        u32x4_t xv[4];
        uint32_t pcx;
        if (c8 + 1 > cap8) { stop = STOP_CF8; break; }
        if constexpr (!bufmode) {
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = cxv[i];
            xb = cxb;
            pcx = cpc;
            s1S = pcx;
            s2S = pcx;
#pragma unroll
            for (int q = 0; q < 8; ++q) xs[q] = (xb >> (7 - q)) & 1u;
            if constexpr (K::passes > 1) {
                // whole-row compares (bf 254) read the element's row from LDS, and slot rows that other waves updated
                // at the end of the previous insertion: one barrier for both
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) *(LA u32x4_t*)(L + f.x + (uint32_t)wave * 64 + i * 16) = xv[i];
                }
                F_LDS_BARRIER();
            }
        } else {
            const size_t ncol = (size_t)e * ((size_t)F + 1) + (size_t)F;
            u64 nraw;
            switch (k.width) {
                case 1: nraw = ldg<uint8_t>(k.bufs + ncol); break;
                case 2: nraw = ldg<uint16_t>(k.bufs + 2 * ncol); break;
                case 4: nraw = ldg<uint32_t>(k.bufs + 4 * ncol); break;
                default: nraw = ldg<u64>(k.bufs + 8 * ncol); break;
            }
            nraw = uni64(nraw);
            if (nraw > 0xFFFFFFFFull) { stop = STOP_RANGE; break; }
            nS = (uint32_t)nraw;
            buf_cols(k.bufs, k.width, e, tid, xs);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                s1S += xs[q];
                s2S += (u64)xs[q] * xs[q];
            }
            xb = centroid_byte(xs, nS);
            *(LA uint8_t*)(L + f.x + tid) = (uint8_t)xb;
            const uint32_t pc = wave_sum63((uint32_t)__popc(xb));
            if (lane == 63) ((LA uint32_t*)(L + f.ppx))[wave] = pc;
            F_LDS_BARRIER();  // the packed centroid and its popcount quarters are visible
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = *(LA u32x4_t*)(L + f.x + (uint32_t)wave * 64 + i * 16);
            const u32x4_t p4 = *(LA u32x4_t*)(L + f.ppx);
            pcx = uni(p4.x + p4.y + p4.z + p4.w);
        }
        FPH(0);
        // ---- greedy descent through the slots (bitbirch.py:305-357) ----------------------------------------
        FPath P;
        P.nd = cRoot; P.D = -1; P.cold = false;
        P.leaflen = 0; P.leafsi = 0; P.leafnode = 0; P.ns_above = 0; P.calls = 0; P.rows_cmp = 0;
        P.leaf.j = 0; P.leaf.link = 0; P.leaf.a = (u32x4_t)(0); P.leaf.b = (u32x4_t)(0);
        // (p_* of level q are written before they are read whenever q < D)
        fast_level<0, K, PROF>(k, L, lv, P, C, xv, pcx, cpar, bpar, pr);
        const int D = P.D;
        cold = P.cold || D < 0;
        const uint32_t jl = P.leaf.j, leaflen = P.leaflen, leafsi = P.leafsi, leafnode = P.leafnode;
        uint32_t (&p_node)[FMAXT] = P.p_node;
        uint32_t (&p_row)[FMAXT] = P.p_row;
        uint32_t (&p_tn)[FMAXT] = P.p_tn;
        uint32_t (&p_si)[FMAXT] = P.p_si;
        FPH(1);
        // ---- the chosen leaf row: its cluster features (the ancestors' are in the register cache) -----------
        const uint32_t Tsub = P.leaf.a.x, slotT = P.leaf.a.z;
        const u64 nT = P.leaf.a.y;
        const u64 s1T = ((u64)P.leaf.b.y << 32) | P.leaf.b.x;
        const u64 s2T = ((u64)P.leaf.b.w << 32) | P.leaf.b.z;
        u32x4_t rawL[2] = {(u32x4_t)(0), (u32x4_t)(0)};
        const uint32_t lbase = f.slot0 + __umul24(leafsi, f.slot_bytes);  // (v_mul_lo_u32 runs at a quarter of the rate)
        // (a BitFeature of one member has its cluster features in its centroid row - this thread's byte of the slot; its
        // reserved uint8 slot may never have been written, see TIER_LAZY)
        const bool singleT = uni((uint32_t)(nT == 1)) != 0;
        if (!cold) {
            if (singleT) rawL[0].x = *(LA uint8_t*)(L + lbase + __umul24(jl, FRBS) + tid);
            else cf_load_raw(k, slotT, tid, rawL);
        }
        const u64 new_n = nT + nS;
        {
            // n_samples of 2^31 and more (anywhere on the path): the complete engine's business (it reports STOP_RANGE
            // beyond 32 bits); below, centroid bits need no 64-bit variant
            uint32_t oflow = new_n > 0x7FFFFFFFull ? 1u : 0u;
            for_levels<0>(D, [&](auto qc) {
                constexpr int q = qc.value;
                oflow |= (p_tn[q] > 0x7FFFFFFFu || nS > 0x7FFFFFFFu - p_tn[q]) ? 1u : 0u;
            });
            if (uni(oflow) != 0) cold = true;
        }
        // ---- one fused pass + one block reduction --------------------------------------------------------------
        const uint32_t tierT = uni(slotT >> 30);
        const bool wide = bufmode || tierT == 2;
        u64 dot = 0;
        uint32_t vL[8], byteL = 0, byteT[FMAXT], pcs[1 + FMAXT];
        static_for<0, 1 + FMAXT>([&](auto i) { pcs[i.value] = 0; });
        static_for<0, FMAXT>([&](auto q) { byteT[q.value] = 0; });
        if (!cold) {
            // the ancestors first: their cluster features are in registers, the leaf row's are still in flight
            for_levels<0>(D, [&](auto qc) {
                constexpr int q = qc.value;
                {
                    uint32_t t[8];
#pragma unroll
                    for (int z = 0; z < 8; ++z) t[z] = C.v[q][z] + xs[z];
                    byteT[q] = centroid_byte_merged31(t, p_tn[q] + nS);
                    pcs[1 + q] = __popc(byteT[q]);
                }
            });
            cf_unpack_raw(singleT ? TIER_LAZY : tierT, rawL, vL);
            if (wide) {
#pragma unroll
                for (int q = 0; q < 8; ++q) dot += (u64)vL[q] * xs[q];
            } else {
                // (uint8 / uint16 cluster features times a bit: 24-bit multiply-adds run at full rate, v_mul_lo_u32 at
                // a quarter of it)
                uint32_t d32 = 0;
#pragma unroll
                for (int q = 0; q < 8; ++q) d32 = __umul24(vL[q], xs[q]) + d32;
                dot = d32;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) vL[q] += xs[q];
            byteL = centroid_byte_merged31(vL, (uint32_t)new_n);
            pcs[0] = __popc(byteL);
        }
        FPH(2);
        {
            // record per wave (12 dwords): [0..1] dot, [2] pc0 | pc1 << 16, [3] pc2 | pc3 << 16, [4] pc4 | pc5 << 16,
            // [5] pc6; BitFeature buffers add [8..9] sum(ls) and [10..11] sum(ls^2) of the element
            uint32_t w2 = pcs[0] | (pcs[1] << 16), w3 = pcs[2] | (pcs[3] << 16), w4 = pcs[4] | (pcs[5] << 16), w5 = pcs[6];
            u64 d = dot, a1 = s1S, a2 = s2S;
            if (wide) d = wave_sum63_64(d);
            else d = wave_sum63((uint32_t)d);
            w2 = wave_sum63(w2);
            if (D > 1) w3 = wave_sum63(w3);
            if (D > 3) w4 = wave_sum63(w4);
            if (D > 5) w5 = wave_sum63(w5);
            if constexpr (bufmode) {
                a1 = wave_sum63_64(a1);
                a2 = wave_sum63_64(a2);
            }
            LA uint32_t* rec = (LA uint32_t*)(L + f.red) + 8;  // records start 32 B into the area (after the fill flags)
            if (lane == 63) {
                u32x4_t r0;
                r0.x = (uint32_t)d; r0.y = (uint32_t)(d >> 32); r0.z = w2; r0.w = w3;
                *(LA u32x4_t*)(rec + wave * 12) = r0;
                u32x2_t r1;
                r1.x = w4; r1.y = w5;
                *(LA u32x2_t*)(rec + wave * 12 + 4) = r1;
                if constexpr (bufmode) {
                    u32x4_t r2;
                    r2.x = (uint32_t)a1; r2.y = (uint32_t)(a1 >> 32); r2.z = (uint32_t)a2; r2.w = (uint32_t)(a2 >> 32);
                    *(LA u32x4_t*)(rec + wave * 12 + 8) = r2;
                }
            }
            F_LDS_BARRIER();
            u64 dsum = 0;
            uint32_t t2 = 0, t3 = 0, t4 = 0, t5 = 0;
            u64 b1 = 0, b2 = 0;
#pragma unroll
            for (int w = 0; w < TW; ++w) {
                const u32x4_t r0 = *(LA u32x4_t*)(rec + w * 12);
                const u32x2_t r1 = *(LA u32x2_t*)(rec + w * 12 + 4);
                dsum += ((u64)r0.y << 32) | r0.x;
                t2 += r0.z; t3 += r0.w; t4 += r1.x; t5 += r1.y;
                if constexpr (bufmode) {
                    const u32x4_t r2 = *(LA u32x4_t*)(rec + w * 12 + 8);
                    b1 += ((u64)r2.y << 32) | r2.x;
                    b2 += ((u64)r2.w << 32) | r2.z;
                }
            }
            dot = dsum;
            pcs[0] = t2 & 0xFFFFu; pcs[1] = t2 >> 16; pcs[2] = t3 & 0xFFFFu; pcs[3] = t3 >> 16;
            pcs[4] = t4 & 0xFFFFu; pcs[5] = t4 >> 16; pcs[6] = t5;
            if constexpr (bufmode) { s1S = b1; s2S = b2; }
        }
        FPH(3);
        // ---- decision (merge criteria of _merges.py on exact moments, float64 in the reference's order) ----------
        const u64 s1n = s1T + s1S;
        const u64 s2n = s2T + 2ull * dot + s2S;
        bool accept = false;
        if (!cold) {
            switch (crit) {
                case BBH_CRIT_DIAMETER:
                    accept = isim_from_moments(s1n, s2n, new_n) >= k.thr;
                    break;
                case BBH_CRIT_TOL_DIAMETER: {
                    const double new_dc = isim_from_moments(s1n, s2n, new_n);
                    if (new_dc < k.thr) accept = false;
                    else if (nT == 1) accept = true;
                    else {
                        // the tolerance table is read-only for the kernel: a scalar load (constant cache), not a
                        // vector-memory round trip in the middle of the decision
                        double told = 0.0;
                        if (k.tol != nullptr && nT < (u64)k.tol_len) {
                            typedef const double __attribute__((address_space(4))) cdouble_t;
                            told = *((cdouble_t*)(uintptr_t)k.tol + uni((uint32_t)nT));
                        }
                        accept = new_dc >= isim_from_moments(s1T, s2T, nT) - told;
                    }
                    break;
                }
                case BBH_CRIT_TOL_LEGACY: {
                    const double new_dc = isim_from_moments(s1n, s2n, new_n);
                    if (new_dc < k.thr) accept = false;
                    else if (nT == 1 || nS != 1) accept = true;
                    else {
                        const double old_dc = isim_from_moments(s1T, s2T, nT);
                        accept = (new_dc * (double)new_n - old_dc * (double)(nT - 1)) / 2 >= old_dc - k.tolerance;
                    }
                    break;
                }
                default: accept = false; break;  // never-merge (radius criteria never reach this kernel)
            }
            accept = uni((uint32_t)accept) != 0;
            if (accept && tier_for(new_n) > tierT) cold = true;        // tier promotion: new CF slot
            if (!accept && tier_for(nS) != 0) cold = true;              // a new BitFeature wider than uint8 (rare)
        }
        // The leaf overflows: split.  In place (cold_leaf_split) when the parent has room, leaf and parent sit in slots the
        // split's scratch does not overlay, and a node + two tracking CFs can be allocated; by the complete engine otherwise.
        bool do_split = false;
        uint32_t sp_node = 0, sp_row = 0, sp_len = 0, sp_si = F_NOSLOT, sp_trk = 0;
        if (!cold && !accept && leaflen + 1 > bf) {
            cold = true;
            static_for<0, FMAXT>([&](auto qc) {
                constexpr int q = qc.value;
                if (q == D - 1) {
                    sp_node = uni(p_node[q]); sp_row = uni(p_row[q]); sp_len = uni(lv.len[q]); sp_si = uni(p_si[q]); sp_trk = uni(P.p_ts[q]);
                }
            });
            if (D >= 1 && sp_len + 1 <= bf && leafsi < (uint32_t)f.cold_slot && (sp_si == F_NOSLOT || sp_si < (uint32_t)f.cold_slot) &&
                uni(lctr[C_NODES]) + K::nblk <= uni(T->cap_nodes) && uni(lctr[C_N32]) + 2 <= uni(T->cap32)) {
                cold = false;
                do_split = true;
            }
        }
        cold = uni((uint32_t)cold) != 0;
        if (cold) break;  // this element goes to the complete engine; nothing of it has been applied
        FPH(5);
        if constexpr (!bufmode) {
            take_prefetched();  // element e+1 is complete in registers before this insertion's stores are issued
            prefetch(e + 2);
        }
        FPH(14);
        // ---- apply ------------------------------------------------------------------------------------------------
        st_calls += P.calls; st_rows += P.rows_cmp;
        st_depth = (uint32_t)(D + 1) > st_depth ? (uint32_t)(D + 1) : st_depth;
        uint32_t out_id;
        const size_t leafm = (size_t)leafnode * NG;
        // Slot updates need no barrier of their own: byte b of a centroid row is written by thread b and read (next
        // compare, phase 1) by the same wave; everything else is read in phase 2, behind that compare's barrier.
        if (accept) {
            // replace_n_samples_and_linear_sum (bitbirch.py:476-484): same tier, same slot (for a BitFeature of one member
            // this is the first time its slot is written)
            uint32_t slotN = slotT;
            if (singleT) slotN = c8++;  // (SLOT_LAZY8: the second member brings the BitFeature its uint8 row)
            cf_store8(k, slotN, tid, vL);
            stg<uint8_t>(k.cent + (leafm + jl) * 256 + tid, (uint8_t)byteL);
            *(LA uint8_t*)(L + lbase + __umul24(jl, FRBS) + tid) = (uint8_t)byteL;
            if (tid == 0) {
                u32x4_t a, b;
                a.x = Tsub; a.y = (uint32_t)new_n; a.z = slotN; a.w = 0;
                b.x = (uint32_t)s1n; b.y = (uint32_t)(s1n >> 32); b.z = (uint32_t)s2n; b.w = (uint32_t)(s2n >> 32);
                stg<u32x4_t>((uint8_t*)(k.rm + leafm + jl), a);
                stg<u32x4_t>((uint8_t*)(k.rm + leafm + jl) + 16, b);
                stg<uint32_t>(k.card + leafm + jl, pcs[0]);
                *(LA u32x4_t*)(L + lbase + f.s_rm + jl * 32) = a;
                *(LA u32x4_t*)(L + lbase + f.s_rm + jl * 32 + 16) = b;
                *(LA uint32_t*)(L + lbase + f.s_card + jl * 4) = pcs[0];
                if (singleT) {
                    stg<uint32_t>(k.link + leafm + jl, slotN);
                    *(LA uint32_t*)(L + lbase + f.s_link + jl * 4) = slotN;
                }
            }
            st_merge += 1;
            out_id = Tsub;
        } else {
            // append_subcluster (bitbirch.py:284-287): a new leaf BitFeature in the next row
            const uint32_t s = cI++;
            // tier 0: n_samples <= 255; a BitFeature of one member has no slot (SLOT_LAZY8: its centroid row is its linear sum)
            uint32_t slotw = SLOT_LAZY8;
            if constexpr (bufmode) {
                if (uni((uint32_t)(nS != 1)) != 0) {
                    slotw = c8++;
                    cf_store8_u8(k, slotw, tid, xs);
                }
            }
            const size_t m = leafm + leaflen;
            stg<uint8_t>(k.cent + m * 256 + tid, (uint8_t)xb);
            *(LA uint8_t*)(L + lbase + __umul24(leaflen, FRBS) + tid) = (uint8_t)xb;
            if (tid == 64) {
                u32x4_t a, b;
                a.x = s; a.y = nS; a.z = slotw; a.w = 0;
                b.x = (uint32_t)s1S; b.y = (uint32_t)(s1S >> 32); b.z = (uint32_t)s2S; b.w = (uint32_t)(s2S >> 32);
                stg<u32x4_t>((uint8_t*)(k.rm + m), a);
                stg<u32x4_t>((uint8_t*)(k.rm + m) + 16, b);
                stg<uint32_t>(k.card + m, pcx);
                stg<uint32_t>(k.link + m, slotw);
                stg<uint32_t>(k.hdr + leafnode, leaflen + 1);
                *(LA u32x4_t*)(L + lbase + f.s_rm + leaflen * 32) = a;
                *(LA u32x4_t*)(L + lbase + f.s_rm + leaflen * 32 + 16) = b;
                *(LA uint32_t*)(L + lbase + f.s_card + leaflen * 4) = pcx;
                *(LA uint32_t*)(L + lbase + f.s_link + leaflen * 4) = slotw;
            }
            static_for<0, FMAXLV>([&](auto q) {
                if (q.value == D) lv.len[q.value] = vpark(leaflen + 1);
            });
            st_append += 1;
            out_id = s;
        }
        // ancestors (closest_subcluster.update, bitbirch.py:352-357): CF += element (in the register cache), new centroid
        const int DU = do_split ? D - 1 : D;  // a split replaces the leaf's own tracking row (bitbirch.py:339-350)
        for_levels<0>(DU, [&](auto qc) {
            constexpr int q = qc.value;
            {
                const size_t pm = (size_t)p_node[q] * NG + p_row[q];
                const uint32_t n_new = p_tn[q] + nS;
#pragma unroll
                for (int z = 0; z < 8; ++z) C.v[q][z] += xs[z];
                stg<uint8_t>(k.cent + pm * 256 + tid, (uint8_t)byteT[q]);
                const bool slotted = uni(p_si[q]) != F_NOSLOT;
                const uint32_t sb = f.slot0 + __umul24(p_si[q] & 0xFFu, f.slot_bytes);
                if (slotted) *(LA uint8_t*)(L + sb + __umul24(p_row[q], FRBS) + tid) = (uint8_t)byteT[q];
                if (tid == 64 * ((q + 1) & 3)) {
                    stg<uint32_t>((uint8_t*)(k.rm + pm) + 4, n_new);
                    stg<uint32_t>(k.card + pm, pcs[1 + q]);
                    if (slotted) {
                        *(LA uint32_t*)(L + sb + f.s_rm + p_row[q] * 32 + 4) = n_new;
                        *(LA uint32_t*)(L + sb + f.s_card + p_row[q] * 4) = pcs[1 + q];
                    }
                }
                if (!slotted) {
                    // tag-only level: its row-0 tracker has changed; a non-zero centroid ends the shortcut
                    lv.tn0[q] = vpark(n_new);
                    if (pcs[1 + q] != 0) lv.tag[q] = vpark(NONE);
                }
            }
        });
        if (tid == 128 && have_out) stg<uint32_t>(out_leaf + e, out_id);
        FPH(4);
        if (do_split) {
            // the parent's tracking CF (without this element, as _split_node's bookkeeping wants it) goes back to HBM
            static_for<0, FMAXT>([&](auto qc) {
                constexpr int q = qc.value;
                if (q == D - 1) {
                    if (uni(C.tag[q]) != NONE) cf_cache_put<q>(k, C);
                    C.tag[q] = vpark(NONE);
                }
            });
            *(LA uint8_t*)(L + f.x + tid) = (uint8_t)xb;  // split_node reads the element's bits from LDS
            // The split itself (cold_leaf_split, a real call) happens in tree_fast_body: a call inside this loop keeps every
            // value that lives across iterations alive across it, and the register allocator answered with stack slots for
            // the level tags - a scratch load + s_waitcnt vmcnt(0) per level of every descent, i.e. a wait for the
            // tracking-CF loads that were meant to overlap the deeper compares.  What survives the split goes to LDS.
            static_for<0, FMAXLV>([&](auto qc) {
                constexpr int q = qc.value;
                if (q == D) lv.tag[q] = vpark(NONE);  // the leaf's rows are redistributed
                if (q == D - 1) {
                    // (both fields written on both paths: an if / else of two stores is merged by the optimiser into ONE
                    // store through a pointer phi, which keeps both level arrays in scratch memory - every tag check of
                    // every descent then is a scratch load behind s_waitcnt vmcnt(0))
                    const bool nos = sp_si == F_NOSLOT;  // tag-only parent: its new rows are not all-zero
                    lv.tag[q] = vpark(nos ? NONE : uni(lv.tag[q]));
                    lv.len[q] = vpark(nos ? uni(lv.len[q]) : sp_len + 1);
                }
                if ((uni(lv.fl[q]) >> 8) != F_NOSLOT && (uni(lv.fl[q]) >> 8) >= (uint32_t)f.cold_slot) lv.tag[q] = vpark(NONE);  // overlaid
            });
            if (tid == 0) {
                LA uint32_t* stash = (LA uint32_t*)(L + f.pp);
                static_for<0, FMAXLV>([&](auto qc) {
                    constexpr int z = qc.value;
                    u32x4_t a;
                    a.x = lv.tag[z]; a.y = lv.len[z]; a.z = lv.fl[z]; a.w = lv.link0[z];
                    u32x2_t b;
                    b.x = lv.ts0[z]; b.y = lv.tn0[z];
                    *(LA u32x4_t*)(stash + z * 8) = a;
                    *(LA u32x2_t*)(stash + z * 8 + 4) = b;
                });
                u32x4_t g0, g1;
                g0.x = nS; g0.y = pcx; g0.z = leafnode; g0.w = leafsi;
                g1.x = sp_node; g1.y = sp_row; g1.z = sp_len; g1.w = sp_si;
                *(LA u32x4_t*)(stash + FMAXLV * 8) = g0;
                *(LA u32x4_t*)(stash + FMAXLV * 8 + 4) = g1;
                stash[FMAXLV * 8 + 8] = sp_trk;
                lctr[12] = 1u;  // tree_fast_body: split pending for element e
            }
            split_exit = true;
            e += 1;
            break;
        }
        e += 1;
    }
    // tracking cluster features go back to HBM before anything else can look at them
    static_for<0, FMAXT>([&](auto q) {
        if (uni(C.tag[q.value]) != NONE) cf_cache_put<q.value>(k, C);
    });
    __syncthreads();
    if (tid0 == 0) {
        lctr[C_IDS] = cI; lctr[C_N8] = c8;
        lctr[8] = (uint32_t)stop;
        lctr[10] = (uint32_t)e; lctr[11] = (uint32_t)((u64)e >> 32);
        lstats[0] += st_calls; lstats[1] += st_rows; lstats[2] += st_merge; lstats[3] += st_append;
        if ((u64)st_depth > lstats[6]) lstats[6] = st_depth;
        if constexpr (PROF) {
            for (int i = 0; i < 16; ++i) T->phase[i] += pr.ph[i];
        }
    }
    __syncthreads();
#undef FPH
    // the element that needs the complete engine / the element after a pending split / done (or stopped: ctr[8])
    return ((cold || split_exit) && stop == STOP_DONE) ? e : n_elems;
}

// one tree per workgroup: the steady-state loop, with the complete engine stepping in for single elements
template <class K, bool PROF>
__device__ __forceinline__ void tree_fast_body(unsigned char* smem_raw, TreeDev* T) {
    constexpr FSmem f = K::f;
    LA unsigned char* L = (LA unsigned char*)smem_raw;
    const int tid = threadIdx.x;
    LA uint32_t* lctr = (LA uint32_t*)(L + f.ctr);
    LA u64* lstats = (LA u64*)(L + f.stats);
    if (tid < C_COUNT) lctr[tid] = T->ctr[tid];
    if (tid == 8) lctr[8] = STOP_DONE;
    if (tid < 8) lstats[tid] = T->stats[tid];
    if (tid < 16) ((LA u32x4_t*)(L + f.x))[tid] = (u32x4_t)(0);
    if (tid < 4) ((LA uint32_t*)(L + f.ppx))[tid] = 0u;
    __syncthreads();
    if (tid == 12) lctr[12] = 0u;
    __syncthreads();
    const long long n_elems = T->n_elems;
    long long e = 0;
    int stop = STOP_DONE;
    bool resume = false;
    while (e < n_elems) {
        e = fast_run<K, PROF>(smem_raw, T, e, resume);
        resume = false;
        stop = (int)uni(lctr[8]);
        if (stop != STOP_DONE) {  // a pool ran full before the element whose index the loop left in ctr[10..11]
            e = (long long)(((u64)uni(lctr[11]) << 32) | uni(lctr[10]));
            break;
        }
        const u64 c0 = PROF ? __builtin_amdgcn_s_memtime() : 0;
        if (uni(lctr[12]) != 0u) {
            // element e - 1 was appended to a leaf that now overflows: split it where it lies (its parent has room), then
            // carry on with the levels above still resident
            LA uint32_t* stash = (LA uint32_t*)(L + f.pp);
            const u32x4_t g0 = *(LA u32x4_t*)(stash + FMAXLV * 8), g1 = *(LA u32x4_t*)(stash + FMAXLV * 8 + 4);
            const uint32_t trk = uni(stash[FMAXLV * 8 + 8]);
            __syncthreads();
            if (tid == 0) lctr[12] = 0u;
            cold_leaf_split<K::BF, PROF>(smem_raw, T, e - 1, uni(g0.x), uni(g0.y), uni(g0.z), uni(g0.w), uni(g1.x), uni(g1.y), uni(g1.z),
                                         uni(g1.w), trk);
            if constexpr (PROF) {
                if (tid == 0) { T->phase[6] += __builtin_amdgcn_s_memtime() - c0; T->phase[7] += 1; }
            }
            const uint32_t sstop = uni(lctr[8]);
            if (sstop != STOP_DONE) { stop = (int)sstop; break; }
            resume = true;
            continue;
        }
        if (e >= n_elems) break;
        cold_insert_one<K::BF>(smem_raw, T, e);
        if constexpr (PROF) {
            if (tid == 0) { T->phase[6] += __builtin_amdgcn_s_memtime() - c0; T->phase[7] += 1; }
        }
        const uint32_t cstop = uni(lctr[8]), cdone = uni(lctr[9]);
        if (tid < 4) ((LA uint32_t*)(L + f.ppx))[tid] = 0u;
        __syncthreads();
        if (cstop != STOP_DONE || cdone == 0) { stop = (int)cstop; break; }
        e += 1;
    }
    __syncthreads();
    if (tid < C_COUNT) T->ctr[tid] = lctr[tid];
    if (tid < 8) T->stats[tid] = lstats[tid];
    if (tid == 0) {
        T->processed = e;
        T->stop_reason = stop;
    }
}

template <class K, bool PROF = false>
__global__ __launch_bounds__(TB) void k_tree_fast(TreeDev* trees) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    tree_fast_body<K, PROF>(smem_raw, trees + blockIdx.x);
}

#endif  // __HIPCC__
