// bb_tree_pipe.inc -- the pipelined insertion kernel (2048-bit packed fingerprints), included by bb_tree.hip.
//
// k_tree_fast inserts ONE element at a time with all four waves in lock step: every phase of an insertion (descent,
// cluster-feature load, reduction, decision, stores) exposes its latency, 9.7 k cycles per insertion on one CU.
// Here the same sequential algorithm (reference bitbirch.py:305-357, :769-787) is a software pipeline of
// SPECIALISED WAVES that keeps several insertions in flight without changing a single decision:
//
//   wave 0, the router:  element e's path through the internal levels.  The levels above the leaf-parent are
//       "zero levels" (every centroid of the node is all-zero: every similarity is 0, np.argmax returns row 0,
//       bitbirch.py:320); their tracking cluster features only receive commutative sums, which are accumulated as
//       bit-sliced counters in registers and added once per run, guarded by the row's exact flip distance (no
//       centroid bit of a zero level can change while the run is in flight).  The leaf-parent P is compared exactly,
//       from an LDS slot; the chosen row's tracking cluster features come from a small LDS cache (32 features per
//       lane) and its new centroid is written back to the slot, so element e+1 is routed against the state element e
//       left behind - while e's leaf phase has not even started.
//   wave 1, the leaf engine: takes routed elements in order from an LDS ring: leaf compare (from its own LDS
//       slots), merge test on exact moments in float64 (the reference's operation order), merge or append,
//       BitFeature ids and cluster-feature slots in insertion order.
//   wave 2: brings the upcoming elements' rows into the ring and PRE-COMPARES them with P's rows: intersections
//       tagged with per-row versions (a seqlock); the router keeps the values whose row has not changed since and
//       recomputes the one or two others - see pipe_choose / pipe_pre.
//   wave 3: pre-compares the leaf engine's queued jobs the same way (nodes of up to 64 rows), or shares the leaf
//       engine's compares and slot fills on request (nodes of 255 rows: four 64-row passes per compare); when
//       every centroid of P is all-zero the router needs no compare and waves 2 and 3 both pre-compare for wave 1.
//
// What makes the overlap exact: the only way e's leaf phase can change what e+1 sees on its way down is a leaf
// split (bitbirch.py:339-350).  The router keeps, per row of P, the child's length and the number of routed
// elements that have not been decided; an element is only released into the ring if its leaf cannot overflow
// even if every element in flight in front of it appends.  An element routed to a FULL leaf is released alone
// and BEFORE any of its tracking updates is applied: merged - the router applies them and carries on; appended
// - the run ends and the leaf is split where it lies (cold_leaf_split_p).  Anything else that might restructure
// the tree above the leaves (a parent without room, exhausted pools, an unstable zero level) ends the run with
// nothing of the element applied: the ring drains, deferred sums are flushed, and the complete engine
// (tree_insert_body<.., ONE>, the cold function k_tree_fast uses) inserts it with HBM current.  Everything the
// leaf engine can meet for a released element (merge, tier promotion, append) it handles itself.
//
// Single-wave ownership: P's slot is written by wave 0 only, the leaf slots by wave 1 only; the waves meet
// through a few LDS words (ring head / tail, results, stamps, row versions), so there is no barrier inside a
// run.  Every wait is bounded (PIPE_SPIN_LIMIT): a wait that gives up raises the abort flag and the launch ends
// with STOP_INTERNAL instead of hanging.

constexpr int PW_MAX = 8;  // entries of the job ring (routed, undecided elements): 8, or 4 for nodes of more than 64 rows
__host__ __device__ constexpr int pipe_pw(int bf) { return bf > 63 ? 4 : 8; }
__host__ __device__ constexpr int pipe_prew(int bf) { return bf > 63 ? 2 : 4; }  // pre-compare buffers in flight
constexpr int PZ = 6;      // zero levels above the leaf-parent handled here
constexpr int PNP = 12;    // bit planes of the deferred zero-level sums: a run takes at most 2^12 - 1 elements
constexpr int PROMO_RESERVE = 1024;  // cf16 / cf32 slots the host guarantees at launch (tier promotions in flight)
constexpr int STOP_PIPE_UNSUPPORTED = 9;  // tree shape the pipeline does not handle: the host runs k_tree_fast for a stretch
constexpr int STOP_INTERNAL = 10;         // a wait inside the pipeline gave up (bug guard: never a hang)
constexpr int STOP_PIPE_NEEDS_ML = 11;    // several exact internal levels: the host relaunches the multi-level instance (K::ML)
constexpr int STOP_PIPE_PREFERS_SL = 12;  // the multi-level instance, after >= PIPE_ML_STINT elements: one exact level again, back to the other instance
#ifndef BBH_ML_STINT
#define BBH_ML_STINT 256
#endif
constexpr long long PIPE_ML_STINT = BBH_ML_STINT;
constexpr int PEMAX = 4;                  // exact internal levels (= upper slots) of the multi-level router (pipe_router_ml)
constexpr uint32_t PRT = 16;              // results of retired jobs the multi-level router remembers (leaf, length)

enum PipeReason : uint32_t { PR_DONE = 0, PR_COLD = 1, PR_STOP = 2, PR_UNSUP = 3, PR_FLUSH = 4, PR_ABORT = 5, PR_SPLIT = 6, PR_NEEDML = 7, PR_PREFSL = 8 };
// split record (u32 indices into the first half of PSmem::mb): what cold_leaf_split_p needs about the leaf that overflowed
enum PipeSplit : int { PS_LEAF = 0, PS_P, PS_JP, PS_LENP, PS_TRK, PS_POP, PS_XOFF, PS_SI };
// control words (u32 indices into PSmem::ctl)
enum PipeCtl : int { PC_HEAD = 0, PC_TAIL, PC_END, PC_ABORT, PC_REASON, PC_E_LO, PC_E_HI, PC_STOPCODE, PC_DCOUNT, PC_NZ, PC_PGO, PC_PLEN, PC_LGO, PC_PZERO,
                     PC_WM,  // (K::ML) the leaf engine's watermark: the global stores of every job below it have completed
                     PC_COUNT };
static_assert(PC_COUNT <= 16, "the control block is 16 words");

struct PSmem {
    uint32_t x, ctr, stats;                // where the cold function expects them (fast_layout's offsets)
    uint32_t ctl, ring, res, xq, delta, zrec;   // xq: the routed elements' packed rows (PW x 256 B)
    uint32_t mb, part;                          // helper mailbox (wave 3 serving wave 1, nodes of > 64 rows) and its partial intersections
    uint32_t srec;                              // split record (PipeSplit)
    uint32_t llog, prec;                        // the leaf slots' change logs, the leaf pre-compares' best rows (pipe_pre_best)
    uint32_t pver, lver, preP, preL, pst;       // row versions of the slots, pre-compare results, stamps (see pipe_prep / pipe_prel)
    int pw, prew;
    uint32_t leaf0, lslot_bytes, s_card, s_link, s_rm;  // leaf slots: the fast kernel's slot layout
    uint32_t pslot, p_card, p_link, p_n, p_ts, p_clen, p_pend, pslot_bytes;  // p_*: relative to pslot
    uint32_t lrest;                        // leaf slots 1 .. nl-1
    uint32_t cold_base, total;
    uint32_t cfc;                          // the leaf engine's cache of uint8 cluster features (ncf x 2 KB; reset every run)
    uint32_t tcf;                          // the router's cache of tracking cluster features (ntc x 8 KB; written back every run)
    int nl, ncf, ntc;
    // multi-level router (K::ML): `nus` slots of pslot_bytes from pslot on (slot 0: the first exact level, the one wave 2
    // pre-compares; the others: an LRU of the nodes below it), the current element's path, the retired jobs' results, the
    // leaf-parent of every ring entry
    int nus;
    uint32_t upath, urt, urp;
};

__host__ __device__ constexpr PSmem pipe_layout(int bf, int ml = 0) {
    PSmem p{};
    const size_t rows = (size_t)bf + 1;
    p.x = 0; p.ctr = 256; p.stats = 256 + 64;
    uint32_t o = 256 + 64 + 64;
    p.ctl = o; o += 64;
    p.pw = pipe_pw(bf); p.prew = pipe_prew(bf);
    const uint32_t lanes4 = (uint32_t)((rows + 63) / 64 * 256);  // one u32 per lane and row pass
    p.ring = o; o += p.pw * 16;
    p.res = o; o += p.pw * 4;
    p.xq = o; o += p.pw * 256;
    p.zrec = o; o += f_align16(PZ * 32);
    p.mb = o; o += 64;
    p.srec = o; o += 32;
    p.pst = o; o += 128;   // u32: [0..3] pstamp, [4..7] ppop, [8..11] lstamp, [16..23] ltag, [24..31] llen
    p.pver = o; o += lanes4;
    p.preP = o; o += p.prew * lanes4;
    p.part = o; o += 2 * (bf > 63 ? lanes4 : 0u);  // (directly behind preP: together they are the four leaf pre-compare buffers of
                                                   //  nodes of > 64 rows while the leaf-parent is all-zero, see pipe_router)
    p.leaf0 = f_align16(o);
    p.s_card = f_align16(rows * FRBS);
    p.s_link = p.s_card + f_align16(rows * 4);
    p.s_rm = p.s_link + f_align16(rows * 4);
    p.lslot_bytes = p.s_rm + (uint32_t)(rows * 32);
    p.cold_base = p.leaf0 + p.lslot_bytes;  // the cold function's scratch overlays everything behind leaf slot 0
    p.pslot = p.cold_base;
    p.delta = p.pslot;  // written when a run ends (the router is done with its slot), read by the flush that follows
    p.p_card = f_align16(rows * FRBS);
    p.p_link = p.p_card + f_align16(rows * 4);
    p.p_n = p.p_link + f_align16(rows * 4);
    p.p_ts = p.p_n + f_align16(rows * 4);
    p.p_clen = p.p_ts + f_align16(rows * 4);
    p.p_pend = p.p_clen + f_align16(rows * 4);
    p.pslot_bytes = p.p_pend + f_align16(rows * 4);
    p.nus = ml ? PEMAX : 1;
    p.lrest = p.pslot + (uint32_t)p.nus * p.pslot_bytes;
    int nl = 1;
    while (nl < (ml ? 3 : 6) && (size_t)p.lrest + (size_t)nl * p.lslot_bytes <= 160 * 1024) ++nl;
    p.nl = nl;
    const uint32_t cold = smem_layout(bf, 256, 0).total;
    const uint32_t end_slots = p.lrest + (uint32_t)(nl - 1) * p.lslot_bytes;
    p.lver = f_align16(end_slots);
    p.preL = bf > 63 ? p.preP : p.lver + (uint32_t)nl * lanes4;
    p.cfc = p.lver + (uint32_t)nl * lanes4 + (bf > 63 ? 0u : (uint32_t)p.prew * lanes4);
    // (what lies behind the caches: the change logs of nodes of several rows per lane, the multi-level router's tables)
    const uint32_t lim = 160 * 1024 - (bf > 63 ? 64u * 7u : 0u) - (ml ? (uint32_t)(PEMAX * 32 + PRT * 8 + PW_MAX * 4 + 64) : 0u);
    int ncf = p.cfc < lim ? (int)((lim - p.cfc) / 2048) : 0;
    p.ncf = ncf > 8 ? 8 : ncf;
    p.tcf = p.cfc + (uint32_t)p.ncf * 2048;
    int ntc = p.tcf < lim ? (int)((lim - p.tcf) / 8192) : 0;
    p.ntc = ntc > 4 ? 4 : (ntc < 0 ? 0 : ntc);
    // (nodes of several rows per lane only, behind everything else)
    p.llog = p.tcf + (uint32_t)p.ntc * 8192;    // per leaf slot: [0] number of row changes so far, [1..8] the rows of the last eight
    p.prec = p.llog + 64 * (uint32_t)nl;        // per leaf pre-compare buffer: {changes seen, best row, its intersection, its key}
    uint32_t end_all = p.prec + 64;
    if (ml) {
        p.upath = end_all;
        p.urt = p.upath + PEMAX * 32;
        p.urp = p.urt + PRT * 8;
        end_all = p.urp + PW_MAX * 4;
    }
    const uint32_t end_cold = p.cold_base + cold;
    p.total = end_all > end_cold ? end_all : end_cold;
    return p;
}

// the part of the layout the complete engine needs for its role as the cold function
__host__ __device__ constexpr FSmem pipe_fsmem(int bf) {
    const PSmem p = pipe_layout(bf);
    FSmem f{};
    f.x = p.x; f.ctr = p.ctr; f.stats = p.stats;
    f.slot0 = p.leaf0; f.slot_bytes = p.lslot_bytes; f.s_card = p.s_card; f.s_link = p.s_link; f.s_rm = p.s_rm;
    f.cold_base = p.cold_base; f.total = p.total; f.ns = p.nl; f.npp = 0; f.cold_slot = 1;
    return f;
}

static_assert(pipe_layout(50).total <= 160 * 1024, "bf 50 must fit");
static_assert(pipe_layout(254).total <= 160 * 1024, "bf 254 must fit");
static_assert(pipe_layout(50, 1).total <= 160 * 1024 && pipe_layout(50, 1).ntc >= 3 && pipe_layout(50, 1).ncf >= 4 && pipe_layout(50, 1).nl >= 3,
              "bf 50, several exact levels: four upper slots, three leaf slots and the caches must fit");
// (the cold functions are compiled per branching factor: both instances must keep x / counters / leaf slot 0 / scratch where they expect them)
static_assert(pipe_layout(50, 1).leaf0 == pipe_layout(50).leaf0 && pipe_layout(50, 1).cold_base == pipe_layout(50).cold_base &&
              pipe_layout(50, 1).lslot_bytes == pipe_layout(50).lslot_bytes, "one cold layout per branching factor");

#if defined(__HIPCC__)

#include "bb_pipe_bytes.h"

#define PIPE_SPIN_LIMIT (1u << 22)
// Where a bounded wait of a launch gave up: the abort flag itself carries the line of this file (any non-zero value aborts),
// the workgroup's thread 0 hands it to the host with STOP_INTERNAL (TreeDev::giveup_line).  Round 4 recorded it with an
// atomicCAS on a device global inside every wait loop: never executed, but the bf 254 instances of the kernel ran 13 % slower
// with it in their loops (S-fake bf 254: 270 k -> 235 k fingerprints/s, bisected to that commit in round 5:
// profiles/r05/bisect_bf254*.txt), the bf 50 instances did not care.
#define PIPE_MARK() ((void)0)
// Run-end audit (phase-timer instances, BBHIP_PIPE_AUDIT=1): when a run has drained, what the waves hold in LDS / registers
// about the nodes they worked on must be what HBM holds - every change is written through.  First difference: check << 16 | line.
//   1 tracking node: a centroid row   2 its popcount   3 its n   4 its child id   5 a child leaf's length   6 jobs still pending
//   7 leaf slot: a centroid row   8 its popcount   9 a row record   10 the leaf's length
__device__ unsigned int g_pipe_audit = 0;
__device__ unsigned long long g_pipe_audit_runs = 0;  // tracking slots + leaf slots audited so far
#define PIPE_AUDIT_FAIL(code) atomicCAS(&g_pipe_audit, 0u, ((unsigned)(code) << 16) | (unsigned)__LINE__)
// LDS executes a wave's accesses in order; this keeps the compiler from moving data accesses across a flag access
#define PIPE_CBAR() asm volatile("" ::: "memory")

template <int BF>
struct KColdP : KCBase {
    static constexpr bool dynamic_shape = false;
    static constexpr int F = 2048, nb = 256, RB = 256, RBc = 16, RBS = (int)FRBS;
    static constexpr uint32_t rows = BF + 1, bf = BF, nblk = node_blocks(BF + 1);
    static constexpr int nm = 1;
    static constexpr Smem o = smem_layout_cold(BF, pipe_fsmem(BF));
};

template <int BF>
__device__ __attribute__((noinline)) void cold_insert_one_p(unsigned char* smem_raw, TreeDev* T, long long e) {
    tree_insert_body<false, KColdP<BF>, true>(smem_raw, T, e);
}

// A leaf that overflowed, split where it lies (_split_node, bitbirch.py:162-211 + update_split_subclusters, :289-303): the
// leaf's rows - the appended element included - are in leaf slot 0, the parent P has room for one more row and is NOT in LDS
// (the split's scratch overlays the router's slot; the next run fills it again).  Same steps as bb_tree_fast.inc's
// cold_leaf_split, on this kernel's layout.
template <int BF, bool PROF = false>
__device__ __attribute__((noinline)) void cold_leaf_split_p(unsigned char* smem_raw, TreeDev* T, long long e, uint32_t pcx, uint32_t leafnode,
                                                            uint32_t P, uint32_t jp, uint32_t lenP, uint32_t trk) {
    const u64 sp_t0 = PROF ? __builtin_amdgcn_s_memtime() : 0;
    constexpr FSmem f = pipe_fsmem(BF);
    KColdS<BF> k;
    k.cent = T->node_cent; k.card = T->node_card; k.link = T->node_link; k.rm = T->node_rm; k.hdr = T->node_hdr;
    k.scratch = T->scratch_cent; k.cf8 = T->cf8; k.cf16 = T->cf16; k.cf32 = T->cf32;
    k.bufs = nullptr; k.width = 0;
    k.crit = 0; k.tol_len = 0; k.thr = 0; k.tolerance = 0; k.tol = nullptr;
    k.L = (LA unsigned char*)smem_raw;
    k.o = smem_layout_cold(BF, f);
    const int tid = threadIdx.x;
    LA uint32_t* lctr = (LA uint32_t*)(k.L + f.ctr);
    LA uint32_t* bc = lds<uint32_t>(k.L, k.o.bc);
    Elem el;
    el.idx = e; el.nS = 1; el.s1S = 0; el.s2S = 0; el.pcx = pcx;
    __syncthreads();
    uint32_t cN = uni(lctr[C_NODES]), c32 = uni(lctr[C_N32]), cFirst = uni(lctr[C_FIRST_LEAF]);
    int red_slot = 0, cmp_par = 0;
    u64 sph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    split_node<false, PROF>(k, el, red_slot, cmp_par, leafnode, 0u, true, trk, cN, c32, cFirst, T->ctr, sph);
    const uint32_t node1 = uni(bc[0]), cardA = uni(bc[3]), cardB = uni(bc[4]);
    const uint32_t nA = uni(bc[7]), nB = uni(bc[8]);
    const uint32_t slotA = (2u << 30) | uni(bc[9]), slotB = (2u << 30) | uni(bc[10]);
    const uint32_t bad = uni(bc[11]);
    // update_split_subclusters (bitbirch.py:289-303): row jp now tracks node1, a new row tracks the split node
    node_put_row(k, P, jp, k.o.cA, cardA, node1, NONE, nA, slotA, 0, 0);
    node_put_row(k, P, lenP, k.o.cB, cardB, leafnode, NONE, nB, slotB, 0, 0);
    if (tid == 0) {
        stg<uint32_t>(k.hdr + P, lenP + 1);
        lctr[C_NODES] = cN; lctr[C_N32] = c32; lctr[C_FIRST_LEAF] = cFirst;
        lctr[8] = bad ? (uint32_t)STOP_RANGE : (uint32_t)STOP_DONE;
    }
    __syncthreads();
    // (the next run starts with empty leaf slots: keeping node1's rows in slot 0 for it was exact but 1.5 % slower at bf 254
    // and 3.8 % at bf 50, profiles/r05/ab_keep.txt)
    if constexpr (PROF) {
        if (tid == 0) {  // (phase-timer build: the split's phases as wave 0 saw them)
            for (int i = 0; i < 8; ++i) T->splitprof[i] += sph[i];
            T->splitprof[8] += 1;
            T->splitprof[9] += __builtin_amdgcn_s_memtime() - sp_t0;
        }
    }
}

template <int BFv, int CRITv, int MLv = 0>
struct KP {
    static constexpr int BF = BFv, CRIT = CRITv;
    static constexpr bool ML = MLv != 0;            // the multi-level router (pipe_router_ml): several exact internal levels
    static constexpr bool HAS_ML = BFv <= 63;        // ... exists for nodes of one row per lane
    static constexpr uint32_t rows = BFv + 1, bf = BFv, nblk = node_blocks(BFv + 1);
    static constexpr int RPL = (BFv + 1 + 63) / 64;  // rows per lane in a node compare
    static constexpr int PW = pipe_pw(BFv), PREW = pipe_prew(BFv);
    // (one leaf engine, helped by pre-compares of the other waves: two leaf engines were exact but 5 % slower, the router is
    // what an insertion waits for - S-fake bf 50 418 k vs 439 k/s, profiles/r04/pipe_phases_variants_1M.txt)
    // Several exact levels (ML): the tracking updates of an element (CF += element, new majority centroid, one per exact
    // level: bitbirch.py:352-357) are done by the HELPER waves - wave 3 the even levels (it does nothing else then: the first
    // level's update is the one the router waits for first; the leaf pre-compares it does otherwise were never used with this
    // router, whose leaf engine is waiting for jobs most of the time), wave 2 the odd ones - while the router goes on with the
    // next element; it waits at every level of the way down until the level's update of the element before is in the slot.
    // See pipe_commit_level / pipe_commit_try.  (The router committing itself was 7 % slower: S-rdkit-like 158 k vs 171 k/s,
    // profiles/r04/fit_workloads_1M.txt.)
#ifndef BBH_PREWL
#define BBH_PREWL 4
#endif
    static constexpr int PREWL = BBH_PREWL;    // leaf pre-compare buffers
    static constexpr PSmem p = pipe_layout(BFv, MLv);
    static_assert(!ML || HAS_ML, "no multi-level instance for this branching factor");
};

__device__ __forceinline__ uint32_t lds_ld(LA unsigned char* L, uint32_t off) { return *(LA volatile uint32_t*)(L + off); }
__device__ __forceinline__ void lds_st(LA unsigned char* L, uint32_t off, uint32_t v) { *(LA volatile uint32_t*)(L + off) = v; }
// four control words in one LDS round trip (a lone wave pays ~110 cycles for every read it waits for): {head, tail, end, abort}
__device__ __forceinline__ u32x4_t lds_ld4(LA unsigned char* L, uint32_t off) { return *(LA volatile u32x4_t*)(L + off); }
static_assert(PC_HEAD == 0 && PC_TAIL == 1 && PC_END == 2 && PC_ABORT == 3, "lds_ld4(ctl) = {head, tail, end, abort}");
// wave 2's stamp of an element it has brought in: the element's number within the run (+ 1: never zero) and its popcount in ONE word
// (a run takes < 2^PNP elements, a 2048-bit row has <= 2048 bits set)
__device__ __forceinline__ uint32_t pipe_stamp(uint32_t i, uint32_t pop) { return (pop << 16) | (i + 1u); }
static_assert(PNP <= 15, "stamp: 16 bits of element number");

// wave-uniform minimum / maximum (SGPR result)
__device__ __forceinline__ uint32_t wmax32(uint32_t v) { return rdlane(wave_max63(v), 63); }
__device__ __forceinline__ uint32_t wmin32(uint32_t v) { return rdlane(wave_min63(v), 63); }

// ---- helper waves -------------------------------------------------------------------------------------------
// Wave 2 serves the router, wave 3 the leaf engine: half of every node compare and of every slot fill, on request
// through a 32-byte LDS mailbox {request seq, op, a0, a1, a2, done seq}.  The master works on its own half meanwhile
// and does not touch the slot before the helper has answered, so the helper reads rows nobody is writing.
enum PipeOp : uint32_t { PO_COMPARE = 1, PO_FILL = 2, PO_EXIT = 3 };

// intersections of the row at `x_off` with this lane's rows of a slot: passes [P0, P1) of 64 rows, 16-byte pieces [C0, C1).
// All pieces of the element's row and of the lane's row are requested before the first popcount (left alone, the compiler
// keeps two reads in flight and waits for each pair: one LDS round trip per piece); with several rows per lane the next
// row's pieces are on their way while this one's are counted.
template <int P0, int P1, int C0, int C1>
__device__ __forceinline__ void pipe_inter(LA unsigned char* L, uint32_t cent_off, uint32_t len, uint32_t x_off, uint32_t (&inter)[P1 > P0 ? P1 - P0 : 1]) {
    constexpr int NP = P1 - P0, NC = C1 - C0;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    const uint32_t last = len - 1;
    uint32_t rb[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const uint32_t r = (uint32_t)(P0 + p) * 64 + lane;
        const uint32_t rc = r < last ? r : last;
        rb[p] = cent_off + __umul24(rc, FRBS) + C0 * 16;
        inter[p] = 0;
    }
    if constexpr (NP == 1 && NC == 16) {
        // one row per lane: two halves of eight pieces (all sixteen at once take 128 registers, and the register allocator
        // then moves the router's loop-carried arrays out of the way and back on every iteration)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            u32x4_t xh[8], dh[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) xh[i] = *(LA u32x4_t*)(L + x_off + (C0 + 8 * h + i) * 16);
#pragma unroll
            for (int i = 0; i < 8; ++i) dh[i] = *(LA u32x4_t*)(L + rb[0] + (8 * h + i) * 16);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int i = 0; i < 8; ++i) inter[0] = popc4v_acc(dh[i] & xh[i], inter[0]);
        }
    } else {
        // (passes whose 64 rows all lie beyond the node's length are skipped: a node of 130 rows is three passes, not four)
        if ((uint32_t)P0 * 64 < len) {
            u32x4_t xq[NC], d[2][NC];
#pragma unroll
            for (int i = 0; i < NC; ++i) xq[i] = *(LA u32x4_t*)(L + x_off + (C0 + i) * 16);
#pragma unroll
            for (int i = 0; i < NC; ++i) d[0][i] = *(LA u32x4_t*)(L + rb[0] + i * 16);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if ((uint32_t)(P0 + p) * 64 < len) {
                    if (p + 1 < NP && (uint32_t)(P0 + p + 1) * 64 < len) {
#pragma unroll
                        for (int i = 0; i < NC; ++i) d[(p + 1) & 1][i] = *(LA u32x4_t*)(L + rb[p + 1 < NP ? p + 1 : p] + i * 16);
                        asm volatile("" ::: "memory");
                    }
#pragma unroll
                    for (int i = 0; i < NC; ++i) inter[p] = popc4v_acc(d[p & 1][i] & xq[i], inter[p]);
                }
            }
        }
    }
}

// how a compare is shared: nodes of up to 64 rows by halves of the row (master pieces 0-7, helper 8-15), larger nodes by
// row passes (master the first half of the passes, helper the rest)
template <int RPL> struct PSplit {
    static constexpr int MP1 = RPL == 1 ? 1 : RPL / 2, HP0 = RPL == 1 ? 0 : RPL / 2;
    static constexpr int MC1 = RPL == 1 ? 8 : 16, HC0 = RPL == 1 ? 8 : 0;
};

__device__ __forceinline__ void pipe_post(LA unsigned char* L, uint32_t mb, uint32_t& seq, uint32_t op, uint32_t a0, uint32_t a1, uint32_t a2) {
    seq += 1;
    if (((uint32_t)ftid() & 63u) == 0) {
        LA volatile uint32_t* m = (LA volatile uint32_t*)(L + mb);
        m[1] = op; m[2] = a0; m[3] = a1; m[4] = a2;
        PIPE_CBAR();
        m[0] = seq;
    }
}
// false: the helper did not answer (abort flag raised)
__device__ __forceinline__ bool pipe_wait_helper(LA unsigned char* L, uint32_t mb, uint32_t seq, uint32_t abort_off) {
    uint32_t spins = 0;
    while (uni(lds_ld(L, mb + 20)) != seq) {
        if (++spins > PIPE_SPIN_LIMIT) { PIPE_MARK(); lds_st(L, abort_off, (uint32_t)__LINE__); return false; }
    }
    PIPE_CBAR();
    return true;
}

// ---- first-argmax of the similarities, from the intersections (one row per lane and pass) --------------------
// Key and tie-break as in bb_tree_fast.inc (sim_key: order-exact float32 quotient; first index among equals, np.argmax).
template <int RPL>
__device__ __forceinline__ void pipe_argmax(LA unsigned char* L, uint32_t card_off, uint32_t len, uint32_t pop, const uint32_t (&inter)[RPL],
                                            uint32_t& j_out, uint32_t& inter_out) {
    const uint32_t lane = (uint32_t)ftid() & 63u;
    const uint32_t last = len - 1;
    uint32_t key[RPL], kloc = 0;
#pragma unroll
    for (int p = 0; p < RPL; ++p) {
        const uint32_t r = (uint32_t)p * 64 + lane;
        const uint32_t rc = r < last ? r : last;
        key[p] = 0u;
        if (p == 0 || (uint32_t)p * 64 < len) {
            const uint32_t card = *(LA uint32_t*)(L + card_off + rc * 4);
            uint32_t un = card + pop - inter[p];
            un = un < 1u ? 1u : un;
            key[p] = r < len ? sim_key(inter[p], un) : 0u;
        }
        kloc = key[p] > kloc ? key[p] : kloc;
    }
    const uint32_t kmax = wmax32(kloc);
    uint32_t j = NONE, it = 0;
#pragma unroll
    for (int p = 0; p < RPL; ++p) {
        const uint32_t r = (uint32_t)p * 64 + lane;
        const u64 m = __ballot(r < len && key[p] == kmax);
        if (j == NONE && m != 0ull) {
            const int l = __ffsll((long long)m) - 1;
            j = (uint32_t)p * 64 + (uint32_t)l;
            it = rdlane(inter[p], l);
        }
    }
    j_out = j;
    inter_out = it;
}

// ---- node compare by the master wave, nodes of > 64 rows shared with its helper (one row per lane: 16-byte column reads at
// the 272-byte row stride are conflict-free, the element's row is a broadcast read) -------------------------------------
template <int RPL>
__device__ __forceinline__ bool pipe_compare(LA unsigned char* L, uint32_t mb, uint32_t part_off, uint32_t abort_off, uint32_t& seq,
                                             uint32_t cent_off, uint32_t card_off, uint32_t len, uint32_t x_off,
                                             uint32_t pop, uint32_t& j_out, uint32_t& inter_out, bool shared) {
    using S = PSplit<RPL>;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    uint32_t inter[RPL];
    bool okh = true;
    if (RPL > 1 && shared) {
        // (the handshake costs what half a 64-row compare does: only nodes of several rows per lane are shared)
        pipe_post(L, mb, seq, PO_COMPARE, cent_off, len, x_off);
        uint32_t own[S::MP1];
        pipe_inter<0, S::MP1, 0, S::MC1>(L, cent_off, len, x_off, own);
#pragma unroll
        for (int p = 0; p < RPL; ++p) inter[p] = p < S::MP1 ? own[p < S::MP1 ? p : 0] : 0u;
        okh = pipe_wait_helper(L, mb, seq, abort_off);
#pragma unroll
        for (int p = S::HP0; p < RPL; ++p) inter[p] += *(LA uint32_t*)(L + part_off + ((uint32_t)p * 64 + lane) * 4);
    } else {
        pipe_inter<0, RPL, 0, 16>(L, cent_off, len, x_off, inter);
    }
    pipe_argmax<RPL>(L, card_off, len, pop, inter, j_out, inter_out);
    return okh;
}

// ---- asynchronous pre-compare --------------------------------------------------------------------------------------------
// A helper wave computes, ahead of time, the intersections of an upcoming element with every row of the slot the chain wave
// will compare it against, and tags every value with the row's VERSION (a per-row counter the slot's owner makes odd before
// it rewrites the row and even again afterwards; the helper reads it before and after the row: a seqlock).  When the
// element's turn comes, the chain wave keeps the values whose version is still the row's current one and recomputes the
// others itself (the rows changed by the few elements in between: usually one or two), 64 lanes on one row.  Same integers,
// same argmax - a stale or torn value is never used.
constexpr uint32_t PRE_INVALID = 0xFFFFFFFFu;

template <int RPL>
__device__ __forceinline__ void pipe_choose(LA unsigned char* L, uint32_t cent_off, uint32_t card_off, uint32_t len, uint32_t pop, uint32_t xd,
                                            uint32_t pre_off, uint32_t ver_off, uint32_t& j_out, uint32_t& inter_out, uint32_t& n_stale) {
    const uint32_t lane = (uint32_t)ftid() & 63u;
    uint32_t inter[RPL];
#pragma unroll
    for (int p = 0; p < RPL; ++p) {
        inter[p] = 0;
        if (p > 0 && (uint32_t)p * 64 >= len) continue;  // (no row of this pass belongs to the node)
        const uint32_t r = (uint32_t)p * 64 + lane;
        const uint32_t en = *(LA uint32_t*)(L + pre_off + r * 4);
        const uint32_t cur = lds_ld(L, ver_off + r * 4);
        inter[p] = en & 0xFFFu;
        const bool valid = en != PRE_INVALID && (en >> 12) == (cur & 0xFFFFFu);
        u64 m = __ballot(r < len && !valid);
        while (m != 0ull) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const uint32_t rr = (uint32_t)p * 64 + (uint32_t)l;
            const uint32_t rowd = *(LA uint32_t*)(L + cent_off + __umul24(rr, FRBS) + lane * 4);
            const uint32_t val = wsum32((uint32_t)__popc(rowd & xd));
            if (lane == (uint32_t)l) inter[p] = val;
            n_stale += 1;
        }
    }
    pipe_argmax<RPL>(L, card_off, len, pop, inter, j_out, inter_out);
}

// A FORWARDED intersection (nodes of one row per lane): the chain wave that has just rewritten a row of its slot already holds
// the next element's row when that element is known, and counts popc(new row & next element) from the registers the row was
// written from - together with the row's popcount, in the same reduction.  The value is kept in the row's lane as
// pipe_fwd(key, value), key = the number (+ 1: never zero) of the element it is for; every other lane holds 0.  The compare of
// exactly that element takes it for that row whatever the pre-compare's tag says: the row has a single writer and is not
// written again before this compare, so it is the integer the `while (m)` loop of pipe_choose would count from LDS.
__device__ __forceinline__ uint32_t pipe_fwd(uint32_t key, uint32_t val) { return (key << 12) | val; }  // (val <= 2048, key < 2^20)

// The same for a node of one row per lane whose owner keeps the rows' popcounts and versions in registers (lane r: row r).
__device__ __forceinline__ void pipe_choose_rv(LA unsigned char* L, uint32_t cent_off, uint32_t len, uint32_t pop, uint32_t xd, uint32_t pre_off,
                                               uint32_t card, uint32_t ver, uint32_t fwd, uint32_t fkey, uint32_t& j_out, uint32_t& inter_out,
                                               uint32_t& n_stale, uint32_t& n_fwd) {
    const uint32_t lane = (uint32_t)ftid() & 63u;
    const uint32_t en = *(LA uint32_t*)(L + pre_off + lane * 4);
    const bool fw = (fwd >> 12) == fkey;
    uint32_t inter = fw ? fwd & 0xFFFu : en & 0xFFFu;
    const bool valid = en != PRE_INVALID && (en >> 12) == (ver & 0xFFFFFu);
    n_fwd += __ballot(fw && !valid) != 0ull ? 1u : 0u;
    u64 m = __ballot(lane < len && !valid && !fw);
    while (m != 0ull) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const uint32_t rowd = *(LA uint32_t*)(L + cent_off + __umul24((uint32_t)l, FRBS) + lane * 4);
        const uint32_t val = wsum32((uint32_t)__popc(rowd & xd));
        if (lane == (uint32_t)l) inter = val;
        n_stale += 1;
    }
    uint32_t un = card + pop - inter;
    un = un < 1u ? 1u : un;
    const uint32_t key = lane < len ? sim_key(inter, un) : 0u;
    const uint32_t kmax = wmax32(key);
    const u64 mm = __ballot(lane < len && key == kmax);
    const int l = __ffsll((long long)mm) - 1;
    j_out = (uint32_t)l;
    inter_out = rdlane(inter, l);
}

// seqlock-tagged intersections of the row at x_off with the rows of a slot -> pre_off
template <int RPL>
__device__ __forceinline__ void pipe_pre(LA unsigned char* L, uint32_t cent_off, uint32_t len, uint32_t x_off, uint32_t ver_off, uint32_t pre_off) {
    const uint32_t lane = (uint32_t)ftid() & 63u;
    uint32_t v1[RPL], inter[RPL];
#pragma unroll
    for (int p = 0; p < RPL; ++p) v1[p] = lds_ld(L, ver_off + ((uint32_t)p * 64 + lane) * 4);
    PIPE_CBAR();
    pipe_inter<0, RPL, 0, 16>(L, cent_off, len, x_off, inter);
    PIPE_CBAR();
#pragma unroll
    for (int p = 0; p < RPL; ++p) {
        const uint32_t r = (uint32_t)p * 64 + lane;
        const uint32_t v2 = lds_ld(L, ver_off + r * 4);
        const bool ok = v1[p] == v2 && (v1[p] & 1u) == 0u && r < len;
        *(LA uint32_t*)(L + pre_off + r * 4) = ok ? ((v1[p] << 12) | inter[p]) : PRE_INVALID;
    }
    PIPE_CBAR();
}

// The leaf engine's variant.  Beyond the tagged values it leaves the FIRST ARGMAX over the rows whose value is valid:
// {c1, row, intersection, key}, c1 = the slot's change count, read by the caller before anything else.  The leaf engine appends the row
// of every change to the slot's log AFTER the row is complete and counts it after that, so a row that is not valid here,
// or that changes later, is among the changes c1+1 .. (count when the element's turn comes): the leaf engine folds those
// rows' current keys into this maximum (pipe_leaf) instead of validating and reducing every row again.
constexpr uint32_t PLOGK = 8;
template <int RPL>
__device__ __forceinline__ void pipe_pre_best(LA unsigned char* L, uint32_t cent_off, uint32_t card_off, uint32_t len, uint32_t x_off, uint32_t pop,
                                              uint32_t ver_off, uint32_t pre_off, uint32_t c1, uint32_t rec_off) {
    const uint32_t lane = (uint32_t)ftid() & 63u;
    const uint32_t last = len - 1;
    uint32_t v1[RPL], inter[RPL], card[RPL];
#pragma unroll
    for (int p = 0; p < RPL; ++p) v1[p] = lds_ld(L, ver_off + ((uint32_t)p * 64 + lane) * 4);
    PIPE_CBAR();
    pipe_inter<0, RPL, 0, 16>(L, cent_off, len, x_off, inter);
#pragma unroll
    for (int p = 0; p < RPL; ++p) {
        const uint32_t r = (uint32_t)p * 64 + lane;
        card[p] = lds_ld(L, card_off + (r < last ? r : last) * 4);
    }
    PIPE_CBAR();
    uint32_t key[RPL], kloc = 0;
    bool ok[RPL];
#pragma unroll
    for (int p = 0; p < RPL; ++p) {
        const uint32_t r = (uint32_t)p * 64 + lane;
        const uint32_t v2 = lds_ld(L, ver_off + r * 4);
        ok[p] = v1[p] == v2 && (v1[p] & 1u) == 0u && r < len;
        *(LA uint32_t*)(L + pre_off + r * 4) = ok[p] ? ((v1[p] << 12) | inter[p]) : PRE_INVALID;
        uint32_t un = card[p] + pop - inter[p];
        un = un < 1u ? 1u : un;
        key[p] = ok[p] ? sim_key(inter[p], un) : 0u;
        kloc = key[p] > kloc ? key[p] : kloc;
    }
    const uint32_t kmax = wmax32(kloc);
    uint32_t j = NONE, it = 0;
#pragma unroll
    for (int p = 0; p < RPL; ++p) {
        const u64 m = __ballot(ok[p] && key[p] == kmax);
        if (j == NONE && m != 0ull) {
            const int l = __ffsll((long long)m) - 1;
            j = (uint32_t)p * 64 + (uint32_t)l;
            it = rdlane(inter[p], l);
        }
    }
    if (lane == 0) {
        u32x4_t rec;
        rec.x = c1; rec.y = j; rec.z = it; rec.w = kmax;
        *(LA u32x4_t*)(L + rec_off) = rec;
    }
    PIPE_CBAR();
}

template <class K>
__device__ __forceinline__ bool pipe_prel_try(LA unsigned char* L, uint32_t& j, uint32_t parity, uint32_t nhelp);

// 32 consecutive features of this lane (features 32 lane .. 32 lane + 31 = the lane's dword of a packed row): bit of feature i
__device__ __forceinline__ uint32_t xbit(uint32_t xd, int i) { return (xd >> (8 * (i >> 3) + 7 - (i & 7))) & 1u; }

// new centroid dword from 32 feature values: bit = v >= ceil(n/2)  (centroid_from_sum, _py_similarity.py:36-41; n >= 2, < 2^31)
__device__ __forceinline__ uint32_t centroid_dword31(const uint32_t (&v)[32], uint32_t n) {
    const uint32_t hm1 = ((n + 1u) >> 1) - 1u;
    uint32_t out = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        uint32_t byte = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) byte = __builtin_amdgcn_alignbit(byte, hm1 - v[8 * b + q], 31);
        out |= (byte & 0xFFu) << (8 * b);
    }
    return out;
}

// ---- tracking updates by the helper waves (K::ML) ------------------------------------------------------------------------
// The mailbox: requests posted by the router (one per routed element: the number of levels, where the element's row is; the
// levels' records {slot, row, cf32 slot word, n before, node} are the router's path entries, p.upath), per helper wave the
// progress word (8 x request + levels of it done: written as soon as the row, its popcount and n are in the slot) and the
// number of requests finished with every store to HBM complete.
enum PipeCq : uint32_t { CQ_SEQ = 0, CQ_N = 2, CQ_XOFF = 3, CQ_PROG = 4, CQ_FIN = 6 };

// a helper wave's part of the LDS cache of tracking cluster features: one or two entries of 8 KB (from p.tcf on), keyed by the
// cf32 slot word.  (Named scalars, not arrays: "the entry that matches" indexed an array at run time and put it in scratch.)
template <int N>
struct PipeTcf {
    static_assert(N == 1 || N == 2, "least recently used = the other one");
    uint32_t tag0, tag1, lru;
    uint32_t done;
    u64 miss;
};
template <int N>
__device__ __forceinline__ void pipe_tcf_init(PipeTcf<N>& st) {
    st.tag0 = NONE; st.tag1 = NONE; st.lru = 0;
    st.done = 0; st.miss = 0;
}
template <class K, int C0, int NC>
__device__ __forceinline__ void pipe_tcf_flush(LA unsigned char* L, TreeDev* T, uint32_t lane, PipeTcf<NC>& st) {
    constexpr PSmem p = K::p;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const uint32_t tg = c == 0 ? st.tag0 : st.tag1;
        if (tg != NONE) {
            uint32_t* dst = T->cf32 + (size_t)(tg & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
#pragma unroll
            for (int g = 0; g < 8; ++g) stg<u32x4_t>(dst + g * 4, *(LA u32x4_t*)(L + p.tcf + (uint32_t)(C0 + c) * 8192 + ((uint32_t)g * 64 + lane) * 16));
        }
    }
    if (lane == 0 && st.miss != 0) atomicAdd((unsigned long long*)&T->mlprof[0], (unsigned long long)st.miss);
}

// One level's tracking row (closest_subcluster.update, bitbirch.py:352-357): CF += element, new centroid.  `rec`: the level's
// path entry.  The progress word is written when the slot holds the new row - the cache and HBM follow.
template <class K, int C0, int NC>
__device__ __forceinline__ void pipe_commit_level(LA unsigned char* L, TreeDev* T, uint32_t lane, PipeTcf<NC>& st, uint32_t rec, uint32_t xd,
                                                  uint32_t prog_off, uint32_t prog_val) {
    constexpr PSmem p = K::p;
    uint32_t* const g_cf32 = T->cf32;
    const u32x4_t a = *(LA u32x4_t*)(L + rec);
    const uint32_t sb = uni(a.x), jl = uni(a.y), tl = uni(a.z), nnew = uni(a.w) + 1u;
    const uint32_t ndl = uni(*(LA uint32_t*)(L + rec + 16));
    uint32_t k = st.tag0 == tl ? 0u : (NC == 2 && st.tag1 == tl ? 1u : NONE);
    uint32_t cf[32];
    if (k == NONE) {
        st.miss += 1;
        k = NC == 2 ? st.lru : 0u;
        const uint32_t oldtag = k == 0u ? st.tag0 : st.tag1;
        st.tag0 = k == 0u ? tl : st.tag0;
        st.tag1 = k == 0u ? st.tag1 : tl;
        const uint32_t* src = g_cf32 + (size_t)(tl & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
        u32x4_t q[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) q[g] = ldg<u32x4_t>(src + g * 4);  // (on its way while the old entry goes back)
        if (oldtag != NONE) {
            uint32_t* dst = g_cf32 + (size_t)(oldtag & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
#pragma unroll
            for (int g = 0; g < 8; ++g) stg<u32x4_t>(dst + g * 4, *(LA u32x4_t*)(L + p.tcf + (C0 + k) * 8192 + ((uint32_t)g * 64 + lane) * 16));
        }
#pragma unroll
        for (int g = 0; g < 8; ++g) { cf[4 * g] = q[g].x; cf[4 * g + 1] = q[g].y; cf[4 * g + 2] = q[g].z; cf[4 * g + 3] = q[g].w; }
    } else {
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const u32x4_t q = *(LA u32x4_t*)(L + p.tcf + (C0 + k) * 8192 + ((uint32_t)g * 64 + lane) * 16);
            cf[4 * g] = q.x; cf[4 * g + 1] = q.y; cf[4 * g + 2] = q.z; cf[4 * g + 3] = q.w;
        }
    }
    st.lru = k ^ 1u;
#pragma unroll
    for (int i = 0; i < 32; ++i) cf[i] += xbit(xd, i);
    const uint32_t cw = centroid_dword31(cf, nnew);
    if (sb == p.pslot) {
        // (slot 0 is pre-compared by wave 2: the row's version is odd while it is being rewritten)
        const uint32_t pv = uni(lds_ld(L, p.pver + jl * 4));
        if (lane == 0) lds_st(L, p.pver + jl * 4, pv + 1);
        PIPE_CBAR();
        *(LA uint32_t*)(L + sb + __umul24(jl, FRBS) + lane * 4) = cw;
        PIPE_CBAR();
        if (lane == 0) lds_st(L, p.pver + jl * 4, pv + 2);
    } else {
        *(LA uint32_t*)(L + sb + __umul24(jl, FRBS) + lane * 4) = cw;
    }
    const uint32_t cardn = wsum32((uint32_t)__popc(cw));
    if (lane == 0) {
        *(LA uint32_t*)(L + sb + p.p_card + jl * 4) = cardn;
        *(LA uint32_t*)(L + sb + p.p_n + jl * 4) = nnew;
    }
    PIPE_CBAR();
    lds_st(L, prog_off, prog_val);
    PIPE_CBAR();
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        u32x4_t q;
        q.x = cf[4 * g]; q.y = cf[4 * g + 1]; q.z = cf[4 * g + 2]; q.w = cf[4 * g + 3];
        *(LA u32x4_t*)(L + p.tcf + (C0 + k) * 8192 + ((uint32_t)g * 64 + lane) * 16) = q;
    }
    const size_t prow = (size_t)ndl * NG + jl;
    stg<uint32_t>(T->node_cent + prow * 256 + lane * 4, cw);
    if (lane == 0) {
        stg<uint32_t>(T->node_card + prow, cardn);
        stg<uint32_t>((uint8_t*)(T->node_rm + prow) + 4, nnew);
    }
}

// The helper wave of parity W (0: wave 3, 1: wave 2): the levels W, W + 2, ... of a request it has not handled yet.  false: none.
template <class K, int W, int C0, int NC>
__device__ __forceinline__ bool pipe_commit_try(LA unsigned char* L, TreeDev* T, uint32_t lane, PipeTcf<NC>& st) {
    constexpr PSmem p = K::p;
    const uint32_t rq = uni(lds_ld(L, p.mb + CQ_SEQ * 4));
    if (rq == st.done) return false;
    PIPE_CBAR();
    const u32x2_t r = *(LA u32x2_t*)(L + p.mb + CQ_N * 4);
    const uint32_t n = uni(r.x), xoff = uni(r.y);
    const uint32_t xd = *(LA uint32_t*)(L + xoff + lane * 4);
    uint32_t k = 0;
#pragma unroll 1
    for (uint32_t l = (uint32_t)W; l < n; l += 2u) {
        k += 1;
        pipe_commit_level<K, C0, NC>(L, T, lane, st, p.upath + l * 32, xd, p.mb + (CQ_PROG + W) * 4, (rq - 1u) * 8u + k);
    }
    // (a node the router brings into a slot later is read from HBM: the request counts as finished when the stores are)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    st.done = rq;
    lds_st(L, p.mb + (CQ_FIN + W) * 4, rq);
    return true;
}

// wave 2: loads the upcoming elements' rows into the ring and pre-compares them with the leaf-parent's rows
template <class K>
__device__ __forceinline__ void pipe_prep(LA unsigned char* L, TreeDev* T, long long e0) {
    constexpr PSmem p = K::p;
    constexpr int RPL = K::RPL;
    constexpr uint32_t LANES4 = (uint32_t)RPL * 256;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    const uint8_t* const in_rows = T->rows;
    const long long row_stride = T->row_stride;
    const long long n_elems = T->n_elems;
    uint32_t spins = 0;
    // the router's go: the slot is filled, versions and stamps are reset
    while (uni(lds_ld(L, p.ctl + PC_PGO * 4)) == 0u) {
        if (uni(lds_ld(L, p.ctl + PC_END * 4)) != 0u || uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) return;
        if (++spins > 64u * PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); return; }
    }
    PIPE_CBAR();
    const uint32_t plen = uni(lds_ld(L, p.ctl + PC_PLEN * 4));
    // every centroid of the leaf-parent all-zero (the router routes to row 0 without comparing, see pipe_router): nothing to
    // pre-compare there, this wave takes the even jobs of the leaf engine's pre-compare instead
    const bool pzero = uni(lds_ld(L, p.ctl + PC_PZERO * 4)) != 0u;
    // stamps / popcounts of the elements brought in: one per pre-compare buffer, or - nothing to pre-compare - the four the
    // stamp area holds, so that this wave can be three elements ahead of the router before it turns to the leaf engine's jobs
    // (with two it kept the router waiting for the next row while it was busy with a 255-row pre-compare)
    const uint32_t nb = pzero ? 4u : (uint32_t)K::PREW;
    static_assert(K::PW >= 4 && K::PREW <= 4, "stamp area: four entries");
    uint32_t i = 0, lj = 0;
    spins = 0;
    // The rows of the next four elements are on their way from HBM before they are needed (one dword per lane and row: four
    // registers): this wave handles one element at a time, and a row requested only when its turn came cost a full memory
    // round trip per element - more than the router needs for an element, which then waited for this wave's stamp
    // ("waiting on the ring" in round 3's phase timers was mostly this).
    auto row_load = [&](uint32_t q) -> uint32_t {
        const long long ee = e0 + (long long)q;
        return ldg<uint32_t>(in_rows + (size_t)(ee < n_elems ? ee : n_elems - 1) * (size_t)row_stride + lane * 4);
    };
    uint32_t xq0 = row_load(0), xq1 = row_load(1), xq2 = row_load(2), xq3 = row_load(3);
    constexpr int NC0 = K::ML ? (p.ntc + 1) / 2 : 1;  // (K::ML) this wave's entries of the cache of tracking cluster features
    PipeTcf<NC0> cst;
    pipe_tcf_init(cst);
#pragma unroll 1
    while (true) {
        if constexpr (K::ML) {
            // a tracking update the router has posted: before anything else (it is waited for)
            if (pipe_commit_try<K, 1, 0, NC0>(L, T, lane, cst)) { spins = 0; continue; }
        }
        const u32x4_t c4 = lds_ld4(L, p.ctl);
        if (uni(c4.z) != 0u || uni(c4.w) != 0u) break;
        const uint32_t h = uni(c4.x), t = uni(c4.y);
        // at most PREW - 1 elements ahead of the router (buffer i % PREW is free once element i - PREW has been routed), and
        // the ring entry must be free (job i - PW done by the leaf engine)
        if (i >= h + (nb - 1u) || i - t >= (uint32_t)K::PW || e0 + (long long)i >= n_elems) {
            if (pzero && uni(lds_ld(L, p.ctl + PC_LGO * 4)) != 0u && pipe_prel_try<K>(L, lj, 0u, 2u)) { spins = 0; continue; }
            if (++spins > 64u * PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); break; }
            continue;
        }
        spins = 0;
        const uint32_t xd = xq0;
        xq0 = xq1; xq1 = xq2; xq2 = xq3;
        xq3 = row_load(i + 4);
        const uint32_t xoff = p.xq + (i & (K::PW - 1)) * 256;
        *(LA uint32_t*)(L + xoff + lane * 4) = xd;
        const uint32_t pop = wsum32((uint32_t)__popc(xd));
        const uint32_t b = i & (nb - 1u);
        if (!pzero) pipe_pre<RPL>(L, p.pslot, plen, xoff, p.pver, p.preP + b * LANES4);
        PIPE_CBAR();
        if (lane == 0) *(LA volatile uint32_t*)(L + p.pst + b * 4) = pipe_stamp(i, pop);
        i += 1;
    }
    // the run is over (the router has seen its last request finished): the cached cluster features go back to HBM
    if constexpr (K::ML) pipe_tcf_flush<K, 0, NC0>(L, T, lane, cst);
}

// One leaf pre-compare, if there is one to do: job j (the next one of this helper's parity that the leaf engine has not
// started, at most PREWL - 1 jobs ahead of it) against the rows of its leaf, when the leaf sits in a slot.  false: nothing to do.
template <class K>
__device__ __forceinline__ bool pipe_prel_try(LA unsigned char* L, uint32_t& j, uint32_t parity, uint32_t nhelp) {
    constexpr PSmem p = K::p;
    constexpr int RPL = K::RPL, NL = p.nl;
    constexpr uint32_t LANES4 = (uint32_t)RPL * 256;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    const uint32_t h = uni(lds_ld(L, p.ctl + PC_HEAD * 4)), t = uni(lds_ld(L, p.ctl + PC_TAIL * 4));
    if (j <= t) j = t + 1;  // the job the leaf engine is working on has been looked at already: stay ahead of it
    if (nhelp == 2 && (j & 1u) != parity) j += 1;
    if (j >= h || j - t >= (uint32_t)K::PREWL) return false;
    PIPE_CBAR();
    const uint32_t leaf = uni(lds_ld(L, p.ring + (j & (K::PW - 1)) * 16 + 4));
    const uint32_t tg = lds_ld(L, p.pst + (16 + (lane < (uint32_t)NL ? lane : 0u)) * 4);
    const u64 m = __ballot(lane < (uint32_t)NL && tg == leaf);
    if (m != 0ull) {  // (not in a slot yet: the leaf engine fills it and compares on its own)
        const uint32_t si = (uint32_t)(__ffsll((long long)m) - 1);
        // (the change count before the length: a row appended in between is then either counted in the length or among the
        // changes the leaf engine looks at again - see pipe_pre_best)
        uint32_t c1 = 0;
        if constexpr (RPL > 1) c1 = uni(lds_ld(L, p.llog + si * 64));
        PIPE_CBAR();
        const uint32_t len = uni(lds_ld(L, p.pst + (24 + si) * 4));
        const uint32_t sb = si == 0 ? p.leaf0 : p.lrest + (si - 1) * p.lslot_bytes;
        const uint32_t b = j & (K::PREWL - 1);
        if (len >= 1) {
            // (nodes of one row per lane: validating and reducing 64 values again costs the leaf engine no more than folding
            // one or two changed rows into the helper's maximum - measured - so the helper only leaves the tagged values)
            if constexpr (RPL == 1) pipe_pre<RPL>(L, sb, len, p.xq + (j & (K::PW - 1)) * 256, p.lver + si * LANES4, p.preL + b * LANES4);
            else pipe_pre_best<RPL>(L, sb, sb + p.s_card, len, p.xq + (j & (K::PW - 1)) * 256, uni(lds_ld(L, p.ring + (j & (K::PW - 1)) * 16 + 12)), p.lver + si * LANES4, p.preL + b * LANES4,
                               c1, p.prec + b * 16);
            if (lane == 0) *(LA volatile uint32_t*)(L + p.pst + (8 + b) * 4) = (j + 1) | (si << 28);
        }
    } else {
        // Not in a slot.  If an earlier job the leaf engine has not finished goes to the same leaf, that job brings it in:
        // come back then (after a split every job of the new run is in this position while the first one fills the slot).
        // Otherwise this job itself will bring it in and compares on its own.
        bool coming = false;
        for (uint32_t q = t; q < j; ++q) coming = coming || uni(lds_ld(L, p.ring + (q & (K::PW - 1)) * 16 + 4)) == leaf;
        if (coming) return false;
    }
    j += 1;
    return true;
}

// a helper wave that only pre-compares for the leaf engine
template <class K>
__device__ __forceinline__ void pipe_prel(LA unsigned char* L, uint32_t parity, uint32_t nhelp) {
    constexpr PSmem p = K::p;
    uint32_t spins = 0;
    while (uni(lds_ld(L, p.ctl + PC_LGO * 4)) == 0u) {
        if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) return;
        if (uni(lds_ld(L, p.ctl + PC_END * 4)) != 0u && uni(lds_ld(L, p.ctl + PC_HEAD * 4)) == 0u) return;
        if (++spins > 64u * PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); return; }
    }
    PIPE_CBAR();
    uint32_t j = 0;
    spins = 0;
#pragma unroll 1
    while (true) {
        if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) break;
        if (pipe_prel_try<K>(L, j, parity, nhelp)) { spins = 0; continue; }
        if (uni(lds_ld(L, p.ctl + PC_END * 4)) != 0u && uni(lds_ld(L, p.ctl + PC_TAIL * 4)) == uni(lds_ld(L, p.ctl + PC_HEAD * 4))) break;
        if (++spins > 64u * PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); break; }
    }
}

// wave 3 of the multi-level instance (K::ML): the even levels' tracking updates
template <class K>
__device__ __forceinline__ void pipe_prel_cmt(LA unsigned char* L, TreeDev* T) {
    constexpr PSmem p = K::p;
    constexpr int NC0 = (p.ntc + 1) / 2, NC1 = K::ML ? p.ntc - NC0 : 1;  // (instantiated for every K, called if K::ML)
    static_assert(NC1 >= 1, "both committing waves need a cache entry");
    const uint32_t lane = (uint32_t)ftid() & 63u;
    PipeTcf<NC1> cst;
    pipe_tcf_init(cst);
    uint32_t spins = 0;
#pragma unroll 1
    while (true) {
        if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) break;
        if (pipe_commit_try<K, 0, NC0, NC1>(L, T, lane, cst)) { spins = 0; continue; }
        // (the router sets the end flag after its last request is finished)
        if (uni(lds_ld(L, p.ctl + PC_END * 4)) != 0u && uni(lds_ld(L, p.ctl + PC_TAIL * 4)) == uni(lds_ld(L, p.ctl + PC_HEAD * 4))) break;
        if (++spins > 64u * PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); break; }
    }
    pipe_tcf_flush<K, NC0, NC1>(L, T, lane, cst);
}

// ---- copy centroid rows of node `nd` into an LDS slot: chunks [I0, I1) of 64 sixteen-byte pieces, requested ahead ------
template <class K, int I0, int I1>
__device__ __forceinline__ void pipe_fill_rows(LA unsigned char* L, uint32_t dst, const uint8_t* cent, uint32_t nd) {
    constexpr uint32_t rows = K::rows;
    constexpr int pieces = (int)rows * 16, NIT = I1 - I0, CH = NIT < 32 ? NIT : 32;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    const uint8_t* src = cent + (size_t)nd * NG * 256;
#pragma unroll 1
    for (int c0 = I0; c0 < I1; c0 += CH) {
        u32x4_t c[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const uint32_t i0 = (uint32_t)(c0 + u) * 64 + lane;
            const uint32_t i = (i0 < (uint32_t)pieces && c0 + u < I1) ? i0 : (uint32_t)pieces - 1;
            c[u] = ldg<u32x4_t>(src + (size_t)i * 16);
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const uint32_t i0 = (uint32_t)(c0 + u) * 64 + lane;
            const uint32_t i = (i0 < (uint32_t)pieces && c0 + u < I1) ? i0 : (uint32_t)pieces - 1;
            *(LA u32x4_t*)(L + dst + (i >> 4) * FRBS + (i & 15) * 16) = c[u];
        }
    }
}
template <class K> struct PFill {
    static constexpr int NIT = ((int)K::rows * 16 + 63) / 64, MID = NIT / 2;
};

// waves 2 and 3
template <class K>
__device__ __forceinline__ void pipe_helper(LA unsigned char* L, TreeDev* T, uint32_t idx) {
    constexpr PSmem p = K::p;
    constexpr int RPL = K::RPL;
    using S = PSplit<RPL>;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    const uint32_t mb = p.mb + idx * 32, part = p.part + idx * (uint32_t)(RPL * 256);
    const uint8_t* const g_cent = T->node_cent;
    uint32_t seq = 0, spins = 0;
#pragma unroll 1
    while (true) {
        const uint32_t rq = uni(lds_ld(L, mb));
        if (rq == seq) {
            if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) break;
            if (++spins > 64u * PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); break; }
            continue;
        }
        spins = 0;
        PIPE_CBAR();
        seq = rq;
        const uint32_t op = uni(lds_ld(L, mb + 4)), a0 = uni(lds_ld(L, mb + 8)), a1 = uni(lds_ld(L, mb + 12)), a2 = uni(lds_ld(L, mb + 16));
        if (op == PO_EXIT) break;
        if (op == PO_COMPARE) {
            uint32_t inter[RPL - S::HP0];
            pipe_inter<S::HP0, RPL, S::HC0, 16>(L, a0, a1, a2, inter);
#pragma unroll
            for (int q = 0; q < RPL - S::HP0; ++q) *(LA uint32_t*)(L + part + ((uint32_t)(S::HP0 + q) * 64 + lane) * 4) = inter[q];
        } else if (op == PO_FILL) {
            pipe_fill_rows<K, PFill<K>::MID, PFill<K>::NIT>(L, a0, g_cent, a1);
        }
        PIPE_CBAR();
        lds_st(L, mb + 20, seq);
    }
}

// (one dword per load: a 16-byte load defines a 4-register tuple, and a loop-carried array that is redefined by tuples in
// one branch and updated register by register elsewhere is not coalesced - it came back as 50 register moves per iteration)
__device__ __forceinline__ void cf32_lane_load(const uint32_t* cf32, uint32_t ts, uint32_t lane, uint32_t (&v)[32]) {
    const uint32_t* src = cf32 + (size_t)(ts & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = ldg<uint32_t>(src + i);
}
__device__ __forceinline__ void cf32_lane_store(uint32_t* cf32, uint32_t ts, uint32_t lane, const uint32_t (&v)[32]) {
    uint32_t* dst = cf32 + (size_t)(ts & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        u32x4_t q;
        q.x = v[4 * i]; q.y = v[4 * i + 1]; q.z = v[4 * i + 2]; q.w = v[4 * i + 3];
        stg<u32x4_t>(dst + i * 4, q);
    }
}



// ---- run-end audit helpers ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t audit_ld(const void* ptr) {  // past this CU's vector cache
    return __hip_atomic_load((const GA uint32_t*)ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the centroid rows of node `nd` as an LDS slot holds them (row r at sb + r * FRBS) against HBM
template <class K>
__device__ __noinline__ void pipe_audit_rows(LA unsigned char* L, const uint8_t* g_cent, uint32_t sb, uint32_t nd, uint32_t len, unsigned code) {
    const uint32_t lane = (uint32_t)ftid() & 63u;
#pragma unroll 1
    for (uint32_t r = 0; r < len; ++r) {
        const uint32_t a = *(LA volatile uint32_t*)(L + sb + r * FRBS + lane * 4);
        const uint32_t b = audit_ld(g_cent + ((size_t)nd * NG + r) * 256 + lane * 4);
        if (__ballot(a != b) != 0ull) { PIPE_AUDIT_FAIL(code); return; }
    }
}
// a tracking node in an upper slot (p_* fields in LDS): rows, popcounts, n, child ids; a leaf-parent: the children's lengths
// (their headers are the leaf engine's stores: issued when its job retired, visible a moment later), nothing pending
template <class K>
__device__ __noinline__ void pipe_audit_tracking_slot(LA unsigned char* L, TreeDev* T, uint32_t sb, uint32_t nd, uint32_t len, bool plevel) {
    constexpr PSmem p = K::p;
    constexpr uint32_t rows = K::rows;
    constexpr int RPL = K::RPL;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    if (lane == 0) atomicAdd(&g_pipe_audit_runs, 1ull);
    pipe_audit_rows<K>(L, T->node_cent, sb, nd, len, 1);
#pragma unroll 1
    for (int q = 0; q < RPL; ++q) {
        const uint32_t r = (uint32_t)q * 64 + lane;
        const bool in = r < len;
        const uint32_t rc = in ? r : 0u;
        const size_t m = (size_t)nd * NG + rc;
        const uint32_t cd = *(LA volatile uint32_t*)(L + sb + p.p_card + rc * 4), nn = *(LA volatile uint32_t*)(L + sb + p.p_n + rc * 4);
        const uint32_t lk = *(LA volatile uint32_t*)(L + sb + p.p_link + rc * 4);
        if (__ballot(in && cd != audit_ld(T->node_card + m)) != 0ull) { PIPE_AUDIT_FAIL(2); return; }
        if (__ballot(in && nn != audit_ld((const uint8_t*)(T->node_rm + m) + 4)) != 0ull) { PIPE_AUDIT_FAIL(3); return; }
        if (__ballot(in && lk != audit_ld(T->node_link + m)) != 0ull) { PIPE_AUDIT_FAIL(4); return; }
        if (plevel) {
            const uint32_t cl = *(LA volatile uint32_t*)(L + sb + p.p_clen + rc * 4), pd = *(LA volatile uint32_t*)(L + sb + p.p_pend + rc * 4);
            if (__ballot(in && pd != 0u) != 0ull) { PIPE_AUDIT_FAIL(6); return; }
            bool bad = true;
            for (int tries = 0; tries < 2000 && bad; ++tries) {
                const uint32_t chw = audit_ld((const uint8_t*)(T->node_hdr + lk) + 4);
                bad = __ballot(in && cl != (hw_cap(chw) < rows ? K::bf + 1 : audit_ld(T->node_hdr + lk))) != 0ull;
                if (bad) __builtin_amdgcn_s_sleep(8);
            }
            if (bad) { PIPE_AUDIT_FAIL(5); return; }
        }
    }
}

// ---- wave 0: the router -----------------------------------------------------------------------------------
struct PProf { u64 ph[16]; u64 mark; };
template <bool PROF>
__device__ __forceinline__ void pph(PProf& pr, int i) {
    if constexpr (PROF) {
        const u64 n = __builtin_amdgcn_s_memtime();
        pr.ph[i] += n - pr.mark;
        pr.mark = n;
    }
}
template <bool PROF>
__device__ __forceinline__ void pph_init(PProf& pr) {
#pragma unroll
    for (int i = 0; i < 16; ++i) pr.ph[i] = 0;
    pr.mark = PROF ? __builtin_amdgcn_s_memtime() : 0;
}
template <bool PROF>
__device__ __forceinline__ void pph_out(const PProf& pr, TreeDev* T, uint32_t lane) {
    if constexpr (PROF) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (pr.ph[i] != 0) atomicAdd((unsigned long long*)&T->phase[i], (unsigned long long)pr.ph[i]);
        }
    }
}

template <class K, bool PROF>
__device__ __forceinline__ void pipe_router(LA unsigned char* L, TreeDev* T, long long e0) {
    PProf pr;
    pph_init<PROF>(pr);
    constexpr PSmem p = K::p;
    constexpr uint32_t rows = K::rows, bf = K::bf;
    constexpr int RPL = K::RPL;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    uint8_t* const g_cent = T->node_cent;
    uint32_t* const g_card = T->node_card;
    uint32_t* const g_link = T->node_link;
    RowMeta* const g_rm = T->node_rm;
    NodeHdr* const g_hdr = T->node_hdr;
    uint32_t* const g_cf32 = T->cf32;
    const long long n_elems = T->n_elems;
    LA uint32_t* lctr = (LA uint32_t*)(L + p.ctr);
    const uint32_t cRoot = uni(lctr[C_ROOT]), depth = uni(lctr[C_DEPTH]);
    const uint32_t c8s = uni(lctr[C_N8]), c16s = uni(lctr[C_N16]), c32s = uni(lctr[C_N32]);
    const uint32_t cap8 = uni(T->cap8), cap16 = uni(T->cap16), cap32 = uni(T->cap32);

    uint32_t reason = PR_DONE, stopcode = STOP_DONE;
    long long e = e0;
    uint32_t used = 0, issued = 0, retired = 0, promos = 0, last_ap = 0, nzc = 0;
    const uint32_t cN0 = uni(lctr[C_NODES]), cap_nodes = uni(T->cap_nodes);
    constexpr uint32_t LANES4 = (uint32_t)RPL * 256;
    uint32_t st_stale = 0;
    u64 rw[4] = {0, 0, 0, 0};  // (phase-timer build) what the router waits for
    (void)rw;
    uint32_t st_calls = 0, st_rows = 0;
    uint32_t dp[PNP];
#pragma unroll
    for (int k = 0; k < PNP; ++k) dp[k] = 0;
    // tracking cluster features of the two rows of the leaf-parent used last (consecutive elements mostly alternate between
    // two or three rows): two register sets X / Y, each with the row it holds and its cf32 slot; `curx`: X was used last.
    // The sets are never copied or swapped (that cost 80 register moves on every control-flow edge around them): the
    // update code exists once per set.
    uint32_t tx[32], ty[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) { tx[i] = 0; ty[i] = 0; }
    uint32_t xtag = NONE, xts = 0, ytag = NONE, yts = 0;
    bool curx = false;
    constexpr int NTC = p.ntc;
    uint32_t ttag[NTC > 0 ? NTC : 1], tts[NTC > 0 ? NTC : 1], tuse[NTC > 0 ? NTC : 1];
#pragma unroll
    for (int c = 0; c < (NTC > 0 ? NTC : 1); ++c) { ttag[c] = NONE; tts[c] = 0; tuse[c] = 0; }

    // ---- the shape of the tree: zero levels along row 0, then the leaf-parent -----------------------------
    uint32_t Z = 0, zrows = 0, P = NONE, plen = 0;
    // Nodes of one row per lane: what the router keeps per row of the leaf-parent - child, tracking n and cluster-feature
    // slot, the child's length and pending jobs, the row's popcount and version - lives in REGISTERS, lane r for row r, and
    // is read with v_readlane.  As LDS words each of them was a round trip of ~110 cycles for this lone wave, a dozen of
    // them per element (round 4's timers: 5.4 k cycles per element, a third of it such round trips); only what another
    // wave reads (the rows, their versions for wave 2) is still written to the slot.
    constexpr bool RV = RPL == 1;
    uint32_t r_link = NONE, r_n = 0, r_ts = 0, r_clen = 0, r_pend = 0, r_card = 0, r_ver = 0;
    uint32_t r_fwd = 0;  // the committed row's intersection with the next element (pipe_fwd), in the row's lane
    uint32_t st_fwd = 0;
    (void)r_link; (void)r_n; (void)r_ts; (void)r_clen; (void)r_pend; (void)r_card; (void)r_ver; (void)r_fwd; (void)st_fwd;
    uint32_t budget = (1u << PNP) - 1;
    bool ok = depth >= 2 && depth - 2 <= (uint32_t)PZ;
    bool needml = false;
    {
        uint32_t nd = cRoot;
#pragma unroll 1
        for (uint32_t z = 0; ok && z + 2 < depth; ++z) {
            // every row of `nd` must have an all-zero centroid; row 0 is where everything goes
            const size_t m = (size_t)nd * NG;
            const uint32_t len = uni(ldg<uint32_t>(g_hdr + nd));
            bool any = false;
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const uint32_t r = (uint32_t)q * 64 + lane;
                const uint32_t rc = r < rows ? r : rows - 1;
                const uint32_t cd = ldg<uint32_t>(g_card + m + rc);
                any = any || (r < len && cd != 0);
            }
            const u32x4_t r0 = ldg<u32x4_t>((const uint8_t*)(g_rm + m));
            const uint32_t l0 = uni(ldg<uint32_t>(g_link + m));
            if (__ballot(any) != 0ull || len == 0) {
                // an informative level above the leaf-parent: the multi-level instance's business where there is one
                if (K::HAS_ML && len != 0) needml = true;
                ok = false;
                break;
            }
            const uint32_t n0 = uni(r0.y), ts0 = uni(r0.z);
            if (n0 >= 0x7FFF0000u) { ok = false; break; }
            // exact flip distance of row 0: min over features of n - 2 ls (all centroid bits are 0, so >= 1); the row
            // stays all-zero for fd - 1 more insertions whatever they are.  Cached across runs with the n it was taken at.
            LA uint32_t* zr = (LA uint32_t*)(L + p.zrec + z * 32);
            uint32_t fd;
            const uint32_t zn = uni(zr[0]), zn_at = uni(zr[2]), zfd = uni(zr[3]);
            if (zn == nd && uni(zr[1]) == ts0 && n0 >= zn_at && zfd > (n0 - zn_at) + 64u) {
                fd = zfd - (n0 - zn_at);
            } else {
                uint32_t v[32];
                cf32_lane_load(g_cf32, ts0, lane, v);
                uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const uint32_t d = 2u * v[i] < n0 ? n0 - 2u * v[i] : 0u;
                    mn = d < mn ? d : mn;
                }
                fd = wmin32(mn);
                if (lane == 0) { zr[2] = n0; zr[3] = fd; }
            }
            if (lane == 0) { zr[0] = nd; zr[1] = ts0; }
            const uint32_t room = fd > 0 ? fd - 1 : 0;
            budget = room < budget ? room : budget;
            zrows += len;
            nd = l0;
            Z = z + 1;
        }
        P = nd;
    }
    if (!ok) {
        reason = needml ? PR_NEEDML : PR_UNSUP;
    } else if (budget == 0) {
        reason = PR_COLD;  // a zero-level centroid may flip with the next insertion: the complete engine's business
    } else {
        // ---- fill P's slot: rows, popcounts, child ids, tracking n / CF slot, the children's lengths ---------------
        const size_t pm = (size_t)P * NG;
        const u32x2_t hraw = ldg<u32x2_t>(g_hdr + P);
        pipe_fill_rows<K, 0, PFill<K>::NIT>(L, p.pslot, g_cent, P);
        uint32_t lk[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const uint32_t r = (uint32_t)q * 64 + lane;
            const uint32_t rc = r < rows ? r : rows - 1;
            const uint32_t cd = ldg<uint32_t>(g_card + pm + rc);
            lk[q] = ldg<uint32_t>(g_link + pm + rc);
            const u32x2_t ns = ldg<u32x2_t>((const uint8_t*)(g_rm + pm + rc) + 4);
            *(LA uint32_t*)(L + p.pslot + p.p_card + rc * 4) = cd;
            *(LA uint32_t*)(L + p.pslot + p.p_link + rc * 4) = lk[q];
            *(LA uint32_t*)(L + p.pslot + p.p_n + rc * 4) = ns.x;
            *(LA uint32_t*)(L + p.pslot + p.p_ts + rc * 4) = ns.y;
            *(LA uint32_t*)(L + p.pslot + p.p_pend + rc * 4) = 0u;
            if constexpr (RV) { r_card = cd; r_link = lk[q]; r_n = ns.x; r_ts = ns.y; r_pend = 0u; r_ver = 0u; }
        }
        plen = uni(hraw.x);
        const bool pleaf = (uni(hraw.y) & HW_LEAF) != 0;
        // (a sealed node - capacity below bf + 1, bb_tree.hip "Node storage" - is thawed by the complete engine before anything is
        // inserted below it; a sealed child counts as a leaf that is more than full, which sends its first element there too)
        const bool psealed = hw_cap(uni(hraw.y)) < rows;
        {
            uint32_t nzl = 0;  // rows of the leaf-parent whose centroid is not all-zero
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const uint32_t r = (uint32_t)q * 64 + lane;
                const uint32_t rc = r < rows ? r : rows - 1;
                nzl += (r < plen && *(LA uint32_t*)(L + p.pslot + p.p_card + rc * 4) != 0u) ? 1u : 0u;
            }
            nzc = wsum32(nzl);
        }
        if (psealed) {
            reason = PR_COLD;
        } else if (pleaf || plen == 0) {
            reason = PR_UNSUP;
        } else {
            bool bad = false;
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const uint32_t r = (uint32_t)q * 64 + lane;
                const uint32_t rc = r < rows ? r : rows - 1;
                uint32_t cl = bf + 1, clf = 1;
                if (r < plen) {
                    const u32x2_t ch = ldg<u32x2_t>(g_hdr + lk[q]);
                    cl = hw_cap(ch.y) < rows ? bf + 1 : ch.x; clf = ch.y & HW_LEAF;
                }
                bad = bad || clf == 0;
                *(LA uint32_t*)(L + p.pslot + p.p_clen + rc * 4) = cl;
                if constexpr (RV) r_clen = cl;
            }
            if (__ballot(bad) != 0ull) reason = PR_UNSUP;  // P's children are not leaves: depth counter and tree disagree
        }
    }

    pph<PROF>(pr, 0);
    if constexpr (PROF) pr.ph[12] += 1;
    const bool pzero = nzc == 0;
    if (reason == PR_DONE) {
        // row versions and stamps start from zero, then wave 2 may go: it loads the elements' rows and pre-compares them
#pragma unroll
        for (int q = 0; q < RPL; ++q) *(LA uint32_t*)(L + p.pver + ((uint32_t)q * 64 + lane) * 4) = 0u;
        if (lane < 8) *(LA uint32_t*)(L + p.pst + lane * 4) = 0u;
        // Every centroid of the leaf-parent all-zero (sparse fingerprints under large branching factors): every similarity is 0 and
        // np.argmax returns row 0 (bitbirch.py:320) - no compare, and wave 2 is free to pre-compare for the leaf engine.  The
        // run ends with the insertion that makes row 0's centroid non-zero.
        if (lane == 0) {
            *(LA uint32_t*)(L + p.ctl + PC_PLEN * 4) = plen;
            *(LA uint32_t*)(L + p.ctl + PC_PZERO * 4) = pzero ? 1u : 0u;
        }
        PIPE_CBAR();
        lds_st(L, p.ctl + PC_PGO * 4, 1u);
        uint32_t tail_seen = 0;
        auto retire_to_tail = [&]() {
            const uint32_t t = tail_seen;  // (read together with the abort flag at the top of the loop, or just now)
            PIPE_CBAR();
            while (retired < t) {
                const uint32_t jj = retired & (K::PW - 1);
                const uint32_t prw = lds_ld(L, p.ring + jj * 16 + 8), apw = lds_ld(L, p.res + jj * 4);  // (both on their way, then both waited for)
                const uint32_t pr = uni(prw) & 0x3FFFFFFFu;
                const uint32_t ap = uni(apw);
                last_ap = ap;
                promos += (ap >> 1) & 1u;
                if constexpr (RV) {
                    r_pend = lane == pr ? r_pend - 1u : r_pend;
                    r_clen = lane == pr ? r_clen + (ap & 1u) : r_clen;
                } else if (lane == 0) {
                    LA uint32_t* pe = (LA uint32_t*)(L + p.pslot + p.p_pend + pr * 4);
                    LA uint32_t* cl = (LA uint32_t*)(L + p.pslot + p.p_clen + pr * 4);
                    *pe = *pe - 1u;
                    *cl = *cl + (ap & 1u);
                }
                retired += 1;
            }
        };
        auto retire_poll = [&]() {
            tail_seen = uni(lds_ld(L, p.ctl + PC_TAIL * 4));
            retire_to_tail();
        };
#pragma unroll 1
        while (true) {
            if (e >= n_elems) { reason = PR_DONE; break; }
            if (used >= budget || (pzero && nzc != 0)) { reason = PR_FLUSH; break; }
            if (c8s + issued + 1 > cap8) { reason = PR_STOP; stopcode = STOP_CF8; break; }
            // (a tier promotion takes a cf16 / cf32 slot: every element in flight may turn out to be one)
            if (c16s + promos + (issued - retired) + 1 > cap16) { reason = PR_STOP; stopcode = STOP_CF16; break; }
            if (c32s + promos + (issued - retired) + 1 > cap32) { reason = PR_STOP; stopcode = STOP_CF32; break; }
            {
                const u32x4_t c4 = lds_ld4(L, p.ctl);  // abort flag and tail in one round trip
                tail_seen = uni(c4.y);
                if (uni(c4.w) != 0u) { reason = PR_ABORT; break; }
            }
            bool give_up = false, full = false;
            u64 wt0 = 0;
            if constexpr (PROF) wt0 = __builtin_amdgcn_s_memtime();
            {
                // a free ring entry first: the element's row goes straight into the entry's 256 bytes (the leaf engine
                // reads it from there), and the compare below reads it back as a broadcast
                uint32_t spins = 0;
                retire_to_tail();
                while (issued - retired >= (uint32_t)K::PW) {
                    __builtin_amdgcn_s_sleep(1);
                    retire_poll();
                    if (++spins > PIPE_SPIN_LIMIT) { give_up = true; PIPE_MARK(); break; }
                }
            }
            if (give_up) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
            if constexpr (PROF) { const u64 n_ = __builtin_amdgcn_s_memtime(); rw[0] += n_ - wt0; wt0 = n_; }
            // the element's row and its pre-compare (wave 2)
            const uint32_t pb = issued & ((pzero ? 4u : (uint32_t)K::PREW) - 1u);  // (see pipe_prep)
            uint32_t stampw = 0;
            {
                uint32_t spins = 0;
                while (((stampw = uni(lds_ld(L, p.pst + pb * 4))) & 0xFFFFu) != issued + 1) {
                    if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u || ++spins > PIPE_SPIN_LIMIT) { give_up = true; PIPE_MARK(); break; }
                }
            }
            if (give_up) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
            PIPE_CBAR();
            if constexpr (PROF) { const u64 n_ = __builtin_amdgcn_s_memtime(); rw[1] += n_ - wt0; }
            pph<PROF>(pr, 1);
            const uint32_t xoff = p.xq + (issued & (K::PW - 1)) * 256;
            const uint32_t xd = *(LA uint32_t*)(L + xoff + lane * 4);
            const uint32_t pop = stampw >> 16;
            uint32_t j, it;
            if (pzero) { j = 0; it = 0; }
            else if constexpr (RV) pipe_choose_rv(L, p.pslot, plen, pop, xd, p.preP + pb * LANES4, r_card, r_ver, r_fwd, issued + 1, j, it, st_stale, st_fwd);
            else pipe_choose<RPL>(L, p.pslot, p.pslot + p.p_card, plen, pop, xd, p.preP + pb * LANES4, p.pver, j, it, st_stale);
            uint32_t leaf, nP, ts;
            if constexpr (RV) {
                leaf = rdlane(r_link, (int)j); nP = rdlane(r_n, (int)j); ts = rdlane(r_ts, (int)j);
            } else {
                leaf = uni(*(LA uint32_t*)(L + p.pslot + p.p_link + j * 4));
                nP = uni(*(LA uint32_t*)(L + p.pslot + p.p_n + j * 4));
                ts = uni(*(LA uint32_t*)(L + p.pslot + p.p_ts + j * 4));
            }
            pph<PROF>(pr, 2);
            if (nP >= 0x7FFF0000u) { reason = PR_COLD; break; }
            // ---- may this element overflow its leaf?  Only released if it cannot, whatever the elements in flight do
            uint32_t cl, pd;
            if constexpr (RV) { cl = rdlane(r_clen, (int)j); pd = rdlane(r_pend, (int)j); }
            else { cl = uni(lds_ld(L, p.pslot + p.p_clen + j * 4)); pd = uni(lds_ld(L, p.pslot + p.p_pend + j * 4)); }
            if constexpr (PROF) wt0 = __builtin_amdgcn_s_memtime();
            if (cl + pd + 1 > bf) {
                uint32_t spins = 0;
                while (pd > 0) {
                    __builtin_amdgcn_s_sleep(1);
                    retire_poll();
                    if constexpr (RV) pd = rdlane(r_pend, (int)j);
                    else pd = uni(lds_ld(L, p.pslot + p.p_pend + j * 4));
                    if (++spins > PIPE_SPIN_LIMIT) { give_up = true; PIPE_MARK(); break; }
                }
                if (give_up) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
                if constexpr (RV) cl = rdlane(r_clen, (int)j);
                else cl = uni(lds_ld(L, p.pslot + p.p_clen + j * 4));
                if (cl + 1 > bf) {
                    // A full leaf.  The leaf engine still gets the element: if it merges, nothing special has happened; if it is
                    // appended, the leaf is split where it lies (cold_leaf_split_p) - provided the parent has room for the new
                    // row and a node and two tracking cluster features can be allocated.  Otherwise: the complete engine, with
                    // nothing of e applied.  Nothing else is routed until this element is decided.
                    // (every element still in flight may take a cf32 slot through a tier promotion: the loop-top check's count)
                    if (cl > bf || plen + 1 > bf || cN0 + K::nblk > cap_nodes || c32s + promos + (issued - retired) + 2 > cap32) { reason = PR_COLD; break; }
                    full = true;
                }
            }
            if constexpr (PROF) { const u64 n_ = __builtin_amdgcn_s_memtime(); rw[2] += n_ - wt0; }
            pph<PROF>(pr, 1);
            // ---- release the element to the leaf engine (its own path is decided; its tracking updates follow below)
            if constexpr (RV) r_pend = lane == j ? r_pend + 1u : r_pend;
            if (lane == 0) {
                if constexpr (!RV) {
                    LA uint32_t* pe = (LA uint32_t*)(L + p.pslot + p.p_pend + j * 4);
                    *pe = *pe + 1u;
                }
                u32x4_t job;
                job.x = (uint32_t)e; job.y = leaf; job.z = j | (full ? 0x80000000u : 0u); job.w = pop;
                *(LA u32x4_t*)(L + p.ring + (issued & (K::PW - 1)) * 16) = job;
            }
            issued += 1;
            PIPE_CBAR();
            lds_st(L, p.ctl + PC_HEAD * 4, issued);
            st_calls += Z + 1;
            st_rows += zrows + plen;
            if (full) {
                if constexpr (PROF) wt0 = __builtin_amdgcn_s_memtime();
                uint32_t spins = 0;
                while (retired != issued) {
                    retire_poll();
                    if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u || ++spins > PIPE_SPIN_LIMIT) { give_up = true; PIPE_MARK(); break; }
                }
                if (give_up) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
                if constexpr (PROF) { const u64 n_ = __builtin_amdgcn_s_memtime(); rw[3] += n_ - wt0; }
                if (last_ap & 1u) {
                    // appended: the leaf holds bf + 1 rows.  The levels above the leaf-parent get the element (deferred sums);
                    // the leaf's own tracking row is replaced by the split (bitbirch.py:339-350) and must reach HBM without it.
                    uint32_t carry = xd;
#pragma unroll
                    for (int k = 0; k < PNP; ++k) {
                        const uint32_t t = dp[k] & carry;
                        dp[k] ^= carry;
                        carry = t;
                    }
                    used += 1;
                    if (lane == 0) {
                        LA uint32_t* sp = (LA uint32_t*)(L + p.srec);
                        sp[PS_LEAF] = leaf; sp[PS_P] = P; sp[PS_JP] = j; sp[PS_LENP] = plen; sp[PS_TRK] = ts; sp[PS_POP] = pop; sp[PS_XOFF] = xoff;
                    }
                    reason = PR_SPLIT;
                    e += 1;
                    break;
                }
            }
            // The next element, if wave 2 has brought it in already (a look, not a wait; the stamp is read before the row it
            // vouches for): its intersection with the row committed below is forwarded to its compare, see pipe_fwd.
            uint32_t nstamp = 0, nxd = 0;
            if constexpr (RV) {
                if (!pzero) {
                    nstamp = lds_ld(L, p.pst + (issued & ((uint32_t)K::PREW - 1u)) * 4);
                    nxd = lds_ld(L, p.xq + (issued & (K::PW - 1)) * 256 + lane * 4);
                }
            }
            // ---- commit.  Zero levels: the element's bits into the bit-sliced deferred sums
            {
                uint32_t carry = xd;
#pragma unroll
                for (int k = 0; k < PNP; ++k) {
                    const uint32_t t = dp[k] & carry;
                    dp[k] ^= carry;
                    carry = t;
                }
                used += 1;
            }
            // the leaf-parent's tracking row (closest_subcluster.update, bitbirch.py:352-357): CF += element, new centroid
            const uint32_t nnew = nP + 1;
            uint32_t cw;
            if constexpr (NTC > 0) {
                // the rows used last keep their tracking cluster features in LDS (entry layout: 16-byte group g of lane l at
                // (g * 64 + l) * 16, conflict-free): nothing of them is carried in registers from one element to the next
                uint32_t k = NONE;
#pragma unroll
                for (int c = 0; c < NTC; ++c)
                    if (ttag[c] == j) k = (uint32_t)c;
                uint32_t cf[32];
                if (k == NONE) {
                    // least recently used entry goes back to HBM, row j's comes in
                    uint32_t best = 0xFFFFFFFFu;
#pragma unroll
                    for (int c = 0; c < NTC; ++c)
                        if (tuse[c] < best) { best = tuse[c]; k = (uint32_t)c; }
                    uint32_t oldtag = NONE, oldts = 0;
#pragma unroll
                    for (int c = 0; c < NTC; ++c)
                        if (k == (uint32_t)c) { oldtag = ttag[c]; oldts = tts[c]; ttag[c] = j; tts[c] = ts; }
                    if (oldtag != NONE) {
                        uint32_t* dst = g_cf32 + (size_t)(oldts & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
#pragma unroll
                        for (int g = 0; g < 8; ++g) stg<u32x4_t>(dst + g * 4, *(LA u32x4_t*)(L + p.tcf + k * 8192 + ((uint32_t)g * 64 + lane) * 16));
                    }
                    const uint32_t* src = g_cf32 + (size_t)(ts & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const u32x4_t q = ldg<u32x4_t>(src + g * 4);
                        cf[4 * g] = q.x; cf[4 * g + 1] = q.y; cf[4 * g + 2] = q.z; cf[4 * g + 3] = q.w;
                    }
                } else {
#pragma unroll
                    for (int g = 0; g < 8; ++g) {
                        const u32x4_t q = *(LA u32x4_t*)(L + p.tcf + k * 8192 + ((uint32_t)g * 64 + lane) * 16);
                        cf[4 * g] = q.x; cf[4 * g + 1] = q.y; cf[4 * g + 2] = q.z; cf[4 * g + 3] = q.w;
                    }
                }
#pragma unroll
                for (int c = 0; c < NTC; ++c)
                    if (k == (uint32_t)c) tuse[c] = used;
#pragma unroll
                for (int i = 0; i < 32; ++i) cf[i] += xbit(xd, i);
                cw = centroid_dword31(cf, nnew);
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    u32x4_t q;
                    q.x = cf[4 * g]; q.y = cf[4 * g + 1]; q.z = cf[4 * g + 2]; q.w = cf[4 * g + 3];
                    *(LA u32x4_t*)(L + p.tcf + k * 8192 + ((uint32_t)g * 64 + lane) * 16) = q;
                }
            } else {
            auto track = [&](uint32_t (&cf)[32], uint32_t& tag, uint32_t& tsl) {
                if (tag != j) {  // this set holds the older row: it goes back to HBM, row j's comes in
                    if (tag != NONE) cf32_lane_store(g_cf32, tsl, lane, cf);
                    // (the loads must not be scheduled above the stores: old and new values would be live together, in
                    // different registers, and every edge around this branch would carry a 32-register copy)
                    asm volatile("" ::: "memory");
                    cf32_lane_load(g_cf32, ts, lane, cf);
                    tag = j;
                    tsl = ts;
                }
#pragma unroll
                for (int i = 0; i < 32; ++i) cf[i] += xbit(xd, i);
                cw = centroid_dword31(cf, nnew);
            };
            if (xtag == j) curx = true;
            else if (ytag == j) curx = false;
            else curx = !curx;  // miss: replace the set that was NOT used last
            if (curx) track(tx, xtag, xts);
            else track(ty, ytag, yts);
            }
            uint32_t cardn;
            if constexpr (RV) {
                // the new row's popcount and its intersection with the next element in one reduction (both <= 2048)
                const uint32_t two = wsum32(((uint32_t)__popc(cw) << 16) | (uint32_t)__popc(cw & nxd));
                cardn = two >> 16;
                const bool known = (uni(nstamp) & 0xFFFFu) == issued + 1;
                r_fwd = known && lane == j ? pipe_fwd(issued + 1, two & 0xFFFFu) : 0u;
            } else {
                cardn = wsum32((uint32_t)__popc(cw));
            }
            const size_t prow = (size_t)P * NG + j;
            // (the row's version is odd while it is being rewritten: wave 2 may be reading it)
            uint32_t pv;
            if constexpr (RV) { pv = rdlane(r_ver, (int)j); r_ver = lane == j ? pv + 2u : r_ver; }
            else pv = uni(lds_ld(L, p.pver + j * 4));
            if (lane == 0) lds_st(L, p.pver + j * 4, pv + 1);
            PIPE_CBAR();
            *(LA uint32_t*)(L + p.pslot + __umul24(j, FRBS) + lane * 4) = cw;
            PIPE_CBAR();
            if (lane == 0) lds_st(L, p.pver + j * 4, pv + 2);
            stg<uint32_t>(g_cent + prow * 256 + lane * 4, cw);
            nzc += cardn != 0 ? 1u : 0u;  // (only ever read while it is 0: exact as a zero test)
            if constexpr (RV) {
                r_card = lane == j ? cardn : r_card;
                r_n = lane == j ? nnew : r_n;
            }
            if (lane == 0) {
                if constexpr (!RV) {
                    *(LA uint32_t*)(L + p.pslot + p.p_card + j * 4) = cardn;
                    *(LA uint32_t*)(L + p.pslot + p.p_n + j * 4) = nnew;
                }
                stg<uint32_t>(g_card + prow, cardn);
                stg<uint32_t>((uint8_t*)(g_rm + prow) + 4, nnew);
            }
            e += 1;
            pph<PROF>(pr, 3);
        }
        if constexpr (PROF) {
            pr.ph[13] += st_stale;
            if (lane == 0) atomicAdd((unsigned long long*)&T->mlprof[6], (unsigned long long)st_fwd);
        }
        // ---- end of the run: the ring drains, deferred state goes where the next reader expects it ---------------
        lds_st(L, p.ctl + PC_END * 4, 1u);
        {
            uint32_t spins = 0;
            while (true) {
                if (uni(lds_ld(L, p.ctl + PC_TAIL * 4)) == issued) break;
                __builtin_amdgcn_s_sleep(1);
                if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) { reason = PR_ABORT; break; }
                if (++spins > PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
            }
        }
        if constexpr (PROF) {
            if (T->audit != 0 && reason != PR_ABORT) {
                // run-end audit: the leaf-parent as this wave holds it against HBM (before the slot becomes the deferred sums' buffer)
                retire_poll();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if constexpr (RV) {
                    if (lane < rows) {
                        *(LA uint32_t*)(L + p.pslot + p.p_card + lane * 4) = r_card;
                        *(LA uint32_t*)(L + p.pslot + p.p_n + lane * 4) = r_n;
                        *(LA uint32_t*)(L + p.pslot + p.p_link + lane * 4) = r_link;
                        *(LA uint32_t*)(L + p.pslot + p.p_clen + lane * 4) = r_clen;
                        *(LA uint32_t*)(L + p.pslot + p.p_pend + lane * 4) = r_pend;
                    }
                }
                PIPE_CBAR();
                // (BBHIP_PIPE_AUDIT=corrupt: the audit auditing itself - one bit of the slot's first row is flipped first)
                if (T->audit == 2 && lane == 0) *(LA uint32_t*)(L + p.pslot) ^= 1u;
                // (a run that ends with a leaf split leaves the full leaf's row to the split: its length is the split's business)
                pipe_audit_tracking_slot<K>(L, T, p.pslot, P, plen, reason != PR_SPLIT);
            }
        }
        if (xtag != NONE) cf32_lane_store(g_cf32, xts, lane, tx);
        if (ytag != NONE) cf32_lane_store(g_cf32, yts, lane, ty);
#pragma unroll
        for (int c = 0; c < NTC; ++c) {
            if (ttag[c] != NONE) {
                uint32_t* dst = g_cf32 + (size_t)(tts[c] & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
#pragma unroll
                for (int g = 0; g < 8; ++g) stg<u32x4_t>(dst + g * 4, *(LA u32x4_t*)(L + p.tcf + (uint32_t)c * 8192 + ((uint32_t)g * 64 + lane) * 16));
            }
        }
#pragma unroll
        for (int k = 0; k < PNP; ++k) *(LA uint32_t*)(L + p.delta + k * 256 + lane * 4) = dp[k];
        pph<PROF>(pr, 4);
    } else {
        lds_st(L, p.ctl + PC_END * 4, 1u);
    }
    if constexpr (PROF) pr.ph[14] += 0;
    (void)st_stale;
    if (lane == 0) {
        LA uint32_t* ctl = (LA uint32_t*)(L + p.ctl);
        ctl[PC_REASON] = reason;
        ctl[PC_E_LO] = (uint32_t)e;
        ctl[PC_E_HI] = (uint32_t)((u64)e >> 32);
        ctl[PC_STOPCODE] = stopcode;
        ctl[PC_DCOUNT] = used;
        ctl[PC_NZ] = Z;
        LA u64* lstats = (LA u64*)(L + p.stats);
        __hip_atomic_fetch_add(lstats + 0, (u64)st_calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(lstats + 1, (u64)st_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (used > 0 && (u64)(Z + 2) > lstats[6]) lstats[6] = Z + 2;
    }
    if constexpr (PROF) {
        if (lane == 0)
            for (int i = 0; i < 4; ++i) atomicAdd((unsigned long long*)&T->rprof[i], (unsigned long long)rw[i]);
    }
    pph_out<PROF>(pr, T, lane);
}

// ---- wave 0 when several internal levels are informative (K::ML) -----------------------------------------------------
// pipe_router handles "zero levels, then the leaf-parent".  Trees over dense or family-structured fingerprints keep
// non-zero centroids further up (S-rdkit-like at bf 50: the leaf-parents' parent; clustered families: every level), and the
// reference compares at every level (bitbirch.py:317-320) and updates every tracking BitFeature on the way back
// (:352-357).  Here the router walks E = depth - 1 - Z exact levels per element, E <= PEMAX:
//   * the first one (`top`, a fixed node while the run lasts) sits in upper slot 0 and is pre-compared by wave 2 exactly
//     as the leaf-parent is in pipe_router;
//   * the nodes below it - different ones from element to element - come through an LRU of the other upper slots
//     (filled from HBM on a miss) and are compared by this wave;
//   * after the element has been released, every level's chosen row gets CF += x and its new centroid, through the cache
//     of tracking cluster features (keyed by the row's cf32 slot), written through to the slot and to HBM - so the next
//     element is routed against the state this one left behind at EVERY level.
// Leaf lengths.  The release rule is pipe_router's (an element is released only if its leaf cannot overflow whatever the
// elements in flight do).  The leaf-parent changes from element to element, so its children's lengths cannot simply live in
// the one slot: a leaf-parent that is (re)filled takes them from the leaves' headers in HBM and corrects them with what
// the header stores may not show yet - the jobs in flight (counted as pending, from the ring) and the jobs that retired
// after the leaf engine's WATERMARK (PC_WM: every global store of the jobs below it has completed; the router keeps the
// last PRT results {leaf, length} and never lets the watermark fall further behind).  While the leaf-parent stays in
// a slot, retiring jobs set its rows' lengths exactly.  Overestimates are possible (a job counted as pending whose append is
// already in the header), underestimates are not; an overestimate only sends the element down the careful path, which
// waits for the leaf's pending jobs and then holds the exact length.
template <class K, bool PROF>
__device__ __forceinline__ void pipe_router_ml(LA unsigned char* L, TreeDev* T, long long e0) {
    PProf pr;
    pph_init<PROF>(pr);
    constexpr PSmem p = K::p;
    constexpr uint32_t rows = K::rows, bf = K::bf;
    static_assert(K::RPL == 1, "nodes of one row per lane");
    constexpr int NUS = p.nus;
    constexpr uint32_t LANES4 = 256;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    uint8_t* const g_cent = T->node_cent;
    uint32_t* const g_card = T->node_card;
    uint32_t* const g_link = T->node_link;
    RowMeta* const g_rm = T->node_rm;
    NodeHdr* const g_hdr = T->node_hdr;
    uint32_t* const g_cf32 = T->cf32;
    const long long n_elems = T->n_elems;
    LA uint32_t* lctr = (LA uint32_t*)(L + p.ctr);
    const uint32_t cRoot = uni(lctr[C_ROOT]), depth = uni(lctr[C_DEPTH]);
    const uint32_t c8s = uni(lctr[C_N8]), c16s = uni(lctr[C_N16]), c32s = uni(lctr[C_N32]);
    const uint32_t cap8 = uni(T->cap8), cap16 = uni(T->cap16), cap32 = uni(T->cap32);
    const uint32_t cN0 = uni(lctr[C_NODES]), cap_nodes = uni(T->cap_nodes);

    uint32_t reason = PR_DONE, stopcode = STOP_DONE;
    long long e = e0;
    uint32_t used = 0, issued = 0, retired = 0, promos = 0, last_ap = 0;
    uint32_t st_stale = 0, st_calls = 0, st_rows = 0;
    u64 fill_cycles = 0, fill_count = 0, tcf_miss = 0, levels = 0;
    (void)fill_cycles; (void)fill_count; (void)tcf_miss; (void)levels;
    uint32_t dp[PNP];
#pragma unroll
    for (int k = 0; k < PNP; ++k) dp[k] = 0;
    // requests posted to the helper waves, the levels of the last one, the levels of it known to be in the slots
    uint32_t cposted = 0, cn_last = 0, cseen = 0;
    bool lost_c = false;
    u64 rw[4] = {0, 0, 0, 0};  // (phase-timer build) what the router waits for, as in pipe_router
    (void)rw;
    u64 cw_cycles = 0, cwa_cycles = 0;  // (phase-timer build) waiting for a level's update / for every update and its stores
    (void)cw_cycles; (void)cwa_cycles;
    auto commit_wait = [&](uint32_t l) {
        if (cposted != 0u && l < cn_last && ((cseen >> l) & 1u) == 0u) {
            const u64 t0_ = PROF ? __builtin_amdgcn_s_memtime() : 0;
            const uint32_t need = (cposted - 1u) * 8u + (l >> 1) + 1u, off = p.mb + (CQ_PROG + (l & 1u)) * 4;
            uint32_t spins = 0;
            while ((int)(uni(lds_ld(L, off)) - need) < 0) {
                if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u || ++spins > PIPE_SPIN_LIMIT) { lost_c = true; PIPE_MARK(); break; }
            }
            PIPE_CBAR();
            cseen |= 1u << l;
            if constexpr (PROF) cw_cycles += __builtin_amdgcn_s_memtime() - t0_;
        }
    };
    auto commit_wait_all = [&]() {
        const u64 t0_ = PROF ? __builtin_amdgcn_s_memtime() : 0;
#pragma unroll
        for (uint32_t w = 0; w < 2; ++w) {
            uint32_t spins = 0;
            while (uni(lds_ld(L, p.mb + (CQ_FIN + w) * 4)) != cposted) {
                if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u || ++spins > PIPE_SPIN_LIMIT) { lost_c = true; PIPE_MARK(); break; }
            }
        }
        PIPE_CBAR();
        cseen = 0xFFu;
        if constexpr (PROF) cwa_cycles += __builtin_amdgcn_s_memtime() - t0_;
    };
    // the upper slots: lane s of these registers describes slot s (node, length, last use)
    uint32_t utag = NONE, ulen = 0, uuse = 0, uclock = 0;

    // ---- the shape of the tree: zero levels along row 0 (as in pipe_router), then E exact levels ---------------------
    uint32_t Z = 0, zrows = 0, top = NONE;
    uint32_t budget = (1u << PNP) - 1;
    bool ok = depth >= 2;
    {
        uint32_t nd = cRoot;
#pragma unroll 1
        for (uint32_t z = 0; ok && z + 2 < depth && z < (uint32_t)PZ; ++z) {
            const size_t m = (size_t)nd * NG;
            const uint32_t len = uni(ldg<uint32_t>(g_hdr + nd));
            const uint32_t rc = lane < rows ? lane : rows - 1;
            const uint32_t cd = ldg<uint32_t>(g_card + m + rc);
            const bool any = lane < len && cd != 0;
            const u32x4_t r0 = ldg<u32x4_t>((const uint8_t*)(g_rm + m));
            const uint32_t l0 = uni(ldg<uint32_t>(g_link + m));
            if (len == 0) { ok = false; break; }
            if (__ballot(any) != 0ull) break;  // the first informative level: exact from here down
            const uint32_t n0 = uni(r0.y), ts0 = uni(r0.z);
            if (n0 >= 0x7FFF0000u) { ok = false; break; }
            LA uint32_t* zr = (LA uint32_t*)(L + p.zrec + z * 32);
            uint32_t fd;
            const uint32_t zn = uni(zr[0]), zn_at = uni(zr[2]), zfd = uni(zr[3]);
            if (zn == nd && uni(zr[1]) == ts0 && n0 >= zn_at && zfd > (n0 - zn_at) + 64u) {
                fd = zfd - (n0 - zn_at);
            } else {
                uint32_t v[32];
                cf32_lane_load(g_cf32, ts0, lane, v);
                uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const uint32_t d = 2u * v[i] < n0 ? n0 - 2u * v[i] : 0u;
                    mn = d < mn ? d : mn;
                }
                fd = wmin32(mn);
                if (lane == 0) { zr[2] = n0; zr[3] = fd; }
            }
            if (lane == 0) { zr[0] = nd; zr[1] = ts0; }
            const uint32_t room = fd > 0 ? fd - 1 : 0;
            budget = room < budget ? room : budget;
            zrows += len;
            nd = l0;
            Z = z + 1;
        }
        top = nd;
    }
    const uint32_t E = ok ? depth - 1 - Z : 0u;  // exact internal levels: `top` ... the leaf-parent

    // Fills upper slot `si` with node `nd`: rows, popcounts, child ids, tracking n / cf32 slot.  `plevel` (the node is a
    // leaf-parent): also its children's lengths, corrected as described above, and their pending counts.  false: the node is
    // not what the depth counter says it should be.
    // (`l`: the level the node is wanted for.)  Everything the slot needs is requested at once - header, rows, per-row words,
    // and as soon as the child ids are back the children's headers - and, in the middle of a run, BEFORE the wait for the
    // helper waves: the only updates whose stores may still be on their way are those of the element before, and of those
    // only the one of this level can be to a node of this depth.  The slot itself is written after the wait: the element
    // before may still be adding to the node it gives up.
    u64 fprof[2] = {0, 0};  // (phase-timer build) a fill's loads / what follows the wait for the helper waves
    (void)fprof;
    bool fill_sealed = false;  // the node fill_slot refused is a sealed one (bb_tree.hip "Node storage"): the complete engine thaws it
    auto fill_slot = [&](uint32_t si, uint32_t nd, bool plevel, bool midrun, uint32_t l) -> bool {
        const uint32_t sb = p.pslot + si * p.pslot_bytes;
        const size_t pm = (size_t)nd * NG;
        bool early = true;
        const u64 ftin = PROF ? __builtin_amdgcn_s_memtime() : 0;
        if (midrun && cposted != 0u && l < cn_last) early = uni(lds_ld(L, p.upath + l * 32 + 16)) != nd;
        if (midrun && !early) commit_wait_all();
        // (the watermark is sampled BEFORE the leaves' headers are requested: what it promises is then in what they return)
        uint32_t wm = 0;
        if (plevel && midrun) {
            wm = uni(lds_ld(L, p.ctl + PC_WM * 4));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        const u64 ft0 = PROF ? __builtin_amdgcn_s_memtime() : 0;
        const u32x2_t hraw = ldg<u32x2_t>(g_hdr + nd);
        const uint32_t rc = lane < rows ? lane : rows - 1;
        const uint32_t lk = ldg<uint32_t>(g_link + pm + rc);
        const uint32_t cd = ldg<uint32_t>(g_card + pm + rc);
        const u32x2_t ns = ldg<u32x2_t>((const uint8_t*)(g_rm + pm + rc) + 4);
        constexpr int NIT = PFill<K>::NIT, pieces = (int)rows * 16;
        static_assert(NIT <= 16, "one batch of row loads");
        u32x4_t c[NIT];
        {
            const uint8_t* src = g_cent + pm * 256;
#pragma unroll
            for (int u = 0; u < NIT; ++u) {
                const uint32_t i0 = (uint32_t)u * 64 + lane;
                c[u] = ldg<u32x4_t>(src + (size_t)(i0 < (uint32_t)pieces ? i0 : (uint32_t)pieces - 1) * 16);
            }
        }
        u64 ch = ((u64)1 << 32) | (u64)(bf + 1);
        if (plevel && lane < uni(hraw.x)) {
            // (written by the leaf engine while the run lasts: read at device scope, past this CU's vector cache)
            ch = __hip_atomic_load((const GA u64*)(g_hdr + lk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if constexpr (PROF) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const u64 n_ = __builtin_amdgcn_s_memtime();
            fprof[0] += n_ - ft0;
        }
        if (midrun && early) commit_wait_all();
        const u64 ft1 = PROF ? __builtin_amdgcn_s_memtime() : 0;
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const uint32_t i0 = (uint32_t)u * 64 + lane;
            const uint32_t i = i0 < (uint32_t)pieces ? i0 : (uint32_t)pieces - 1;
            *(LA u32x4_t*)(L + sb + (i >> 4) * FRBS + (i & 15) * 16) = c[u];
        }
        *(LA uint32_t*)(L + sb + p.p_card + rc * 4) = cd;
        *(LA uint32_t*)(L + sb + p.p_link + rc * 4) = lk;
        *(LA uint32_t*)(L + sb + p.p_n + rc * 4) = ns.x;
        *(LA uint32_t*)(L + sb + p.p_ts + rc * 4) = ns.y;
        const uint32_t len = uni(hraw.x);
        const bool isleaf = (uni(hraw.y) & HW_LEAF) != 0;
        if (hw_cap(uni(hraw.y)) < rows) {
            fill_sealed = true;
            utag = lane == si ? NONE : utag;
            return false;
        }
        utag = lane == si ? nd : utag;
        ulen = lane == si ? len : ulen;
        if (isleaf || len == 0) return false;
        if (plevel) {
            uint32_t cl = (uint32_t)ch, pd = 0;
            const uint32_t clf = (uint32_t)(ch >> 32);
            if (__ballot((clf & HW_LEAF) == 0) != 0ull) return false;  // its children are not leaves
            if (lane < len && hw_cap(clf) < rows) cl = bf + 1;  // (a sealed leaf: more than full - its first element goes to the complete engine)
            if (midrun) {
                // results of retired jobs the leaves' headers may not show yet (oldest first: lengths only grow within a run)
                for (uint32_t q = wm; q < retired; ++q) {
                    const u32x2_t rr = *(LA u32x2_t*)(L + p.urt + (q & (PRT - 1)) * 8);
                    const uint32_t lf = uni(rr.x), ln = uni(rr.y);
                    if (lane < len && lk == lf && ln > cl) cl = ln;
                }
                // jobs in flight
                for (uint32_t q = retired; q < issued; ++q) {
                    const uint32_t lf = uni(lds_ld(L, p.ring + (q & (K::PW - 1)) * 16 + 4));
                    if (lane < len && lk == lf) pd += 1;
                }
            }
            *(LA uint32_t*)(L + sb + p.p_clen + rc * 4) = cl;
            *(LA uint32_t*)(L + sb + p.p_pend + rc * 4) = pd;
        }
        if constexpr (PROF) {
            const u64 n_ = __builtin_amdgcn_s_memtime();
            fprof[1] += n_ - ft1;
            if (midrun) fill_cycles += n_ - ftin;
        }
        return true;
    };

    if (!ok || E == 0 || E > (uint32_t)NUS) {
        reason = PR_UNSUP;
    } else if (E == 1 && e0 >= PIPE_ML_STINT) {
        // Zero levels, then the leaf-parent: the single-level instance's shape, and it is a third faster on it (S-fake, bf 50:
        // 450 k against 339 k fingerprints/s).  Informative levels further up come and go - a tracking row of a node that has
        // just been split counts few members, its majority centroid is not all-zero yet - so the tree moves between the two
        // instances; a stint here lasts at least PIPE_ML_STINT elements, which bounds what the relaunches cost.
        reason = PR_PREFSL;
    } else if (budget == 0) {
        reason = PR_COLD;  // a zero-level centroid may flip with the next insertion: the complete engine's business
    } else if (!fill_slot(0, top, E == 1, false, 0u)) {
        reason = fill_sealed ? PR_COLD : PR_UNSUP;
    }
    const uint32_t plen0 = (uint32_t)__builtin_amdgcn_readlane((int)ulen, 0);
    pph<PROF>(pr, 0);
    if constexpr (PROF) pr.ph[12] += 1;
    if (reason == PR_DONE) {
        *(LA uint32_t*)(L + p.pver + lane * 4) = 0u;
        if (lane < 8) *(LA uint32_t*)(L + p.pst + lane * 4) = 0u;
        if (lane == 0) {
            *(LA uint32_t*)(L + p.ctl + PC_PLEN * 4) = plen0;
            *(LA uint32_t*)(L + p.ctl + PC_PZERO * 4) = 0u;
        }
        PIPE_CBAR();
        lds_st(L, p.ctl + PC_PGO * 4, 1u);
        bool lost = false;
        auto retire_poll = [&]() {
            const uint32_t t = uni(lds_ld(L, p.ctl + PC_TAIL * 4));
            PIPE_CBAR();
            while (retired < t) {
                const uint32_t jj = retired & (K::PW - 1);
                const uint32_t prow = uni(lds_ld(L, p.ring + jj * 16 + 8)) & 0x7FFFFFFFu;
                const uint32_t lf = uni(lds_ld(L, p.ring + jj * 16 + 4));
                const uint32_t pn = uni(lds_ld(L, p.urp + jj * 4));
                const uint32_t ap = uni(lds_ld(L, p.res + jj * 4));
                last_ap = ap;
                promos += (ap >> 1) & 1u;
                const uint32_t ln = ap >> 8;
                // (the record entry that is overwritten belongs to job retired - PRT: it must be below the watermark)
                uint32_t spins = 0;
                while (retired >= PRT && uni(lds_ld(L, p.ctl + PC_WM * 4)) + PRT <= retired) {
                    if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u || ++spins > PIPE_SPIN_LIMIT) { lost = true; PIPE_MARK(); break; }
                }
                if (lost) break;
                const u64 m = __ballot(lane < (uint32_t)NUS && utag == pn);
                if (lane == 0) {
                    if (m != 0ull) {
                        const uint32_t sb = p.pslot + (uint32_t)(__ffsll((long long)m) - 1) * p.pslot_bytes;
                        LA uint32_t* pe = (LA uint32_t*)(L + sb + p.p_pend + prow * 4);
                        *pe = *pe - 1u;
                        *(LA uint32_t*)(L + sb + p.p_clen + prow * 4) = ln;
                    }
                    u32x2_t rr;
                    rr.x = lf; rr.y = ln;
                    *(LA u32x2_t*)(L + p.urt + (retired & (PRT - 1)) * 8) = rr;
                }
                retired += 1;
            }
        };
#pragma unroll 1
        while (true) {
            if (e >= n_elems) { reason = PR_DONE; break; }
            if (used >= budget) { reason = PR_FLUSH; break; }
            if (c8s + issued + 1 > cap8) { reason = PR_STOP; stopcode = STOP_CF8; break; }
            if (c16s + promos + (issued - retired) + 1 > cap16) { reason = PR_STOP; stopcode = STOP_CF16; break; }
            if (c32s + promos + (issued - retired) + 1 > cap32) { reason = PR_STOP; stopcode = STOP_CF32; break; }
            if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) { reason = PR_ABORT; break; }
            bool give_up = false, full = false;
            u64 wt0 = PROF ? __builtin_amdgcn_s_memtime() : 0;
            {
                uint32_t spins = 0;
                retire_poll();
                while (!lost && issued - retired >= (uint32_t)K::PW) {
                    __builtin_amdgcn_s_sleep(1);
                    retire_poll();
                    if (++spins > PIPE_SPIN_LIMIT) { give_up = true; PIPE_MARK(); break; }
                }
            }
            if (give_up || lost) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
            if constexpr (PROF) { const u64 n_ = __builtin_amdgcn_s_memtime(); rw[0] += n_ - wt0; wt0 = n_; }
            const uint32_t pb = issued & ((uint32_t)K::PREW - 1u);
            uint32_t stampw = 0;
            {
                uint32_t spins = 0;
                while (((stampw = uni(lds_ld(L, p.pst + pb * 4))) & 0xFFFFu) != issued + 1) {
                    if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u || ++spins > PIPE_SPIN_LIMIT) { give_up = true; PIPE_MARK(); break; }
                }
            }
            if (give_up) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
            PIPE_CBAR();
            if constexpr (PROF) { const u64 n_ = __builtin_amdgcn_s_memtime(); rw[1] += n_ - wt0; }
            pph<PROF>(pr, 1);
            const uint32_t xoff = p.xq + (issued & (K::PW - 1)) * 256;
            const uint32_t xd = *(LA uint32_t*)(L + xoff + lane * 4);
            const uint32_t pop = stampw >> 16;
            // ---- the element's way down: one exact level after the other -------------------------------------------
            uint32_t nd = top, used_mask = 0, rows_e = 0;
            uint32_t sbP = 0, j = 0, ts = 0, plen = 0, Pn = top, leaf = NONE;
            bool bail = false;
#pragma unroll 1
            for (uint32_t l = 0; l < E; ++l) {
                uint32_t si = 0;
                if (l != 0) {
                    const u64 m = __ballot(lane < (uint32_t)NUS && utag == nd);
                    if (m != 0ull) {
                        si = (uint32_t)(__ffsll((long long)m) - 1);
                    } else {
                        // least recently used slot that is not on this element's path (slot 0 belongs to `top`)
                        const bool cand = lane >= 1 && lane < (uint32_t)NUS && ((used_mask >> lane) & 1u) == 0u;
                        const uint32_t vmin = wmin32(cand ? uuse : 0xFFFFFFFFu);
                        si = (uint32_t)(__ffsll((long long)__ballot(cand && uuse == vmin)) - 1);
                        retire_poll();  // (the corrections of a refilled leaf-parent start from the current tail)
                        if (lost) { bail = true; reason = PR_ABORT; break; }
                        const bool filled = fill_slot(si, nd, l + 1 == E, true, l);
                        if (lost_c) { bail = true; reason = PR_ABORT; break; }
                        if (!filled) { bail = true; reason = fill_sealed ? PR_COLD : PR_UNSUP; break; }
                        if constexpr (PROF) fill_count += 1;  // (their cycles: counted in fill_slot, part of the compare phase)
                    }
                }
                used_mask |= 1u << si;
                uclock += 1;
                uuse = lane == si ? uclock : uuse;
                const uint32_t sb = p.pslot + si * p.pslot_bytes;
                const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)ulen, (int)si);
                uint32_t jj, it;
                commit_wait(l);  // (the element before: its update of this level - maybe of a row of this slot)
                if (lost_c) { bail = true; reason = PR_ABORT; break; }
                if (l == 0) {
                    pipe_choose<1>(L, sb, sb + p.p_card, len, pop, xd, p.preP + pb * LANES4, p.pver, jj, it, st_stale);
                } else {
                    uint32_t inter[1];
                    pipe_inter<0, 1, 0, 16>(L, sb, len, xoff, inter);
                    pipe_argmax<1>(L, sb + p.p_card, len, pop, inter, jj, it);
                }
                const uint32_t lk = uni(*(LA uint32_t*)(L + sb + p.p_link + jj * 4));
                const uint32_t nn = uni(*(LA uint32_t*)(L + sb + p.p_n + jj * 4));
                const uint32_t tt = uni(*(LA uint32_t*)(L + sb + p.p_ts + jj * 4));
                if (nn >= 0x7FFF0000u) { bail = true; reason = PR_COLD; break; }
                if (lane == 0) {
                    u32x4_t a;
                    a.x = sb; a.y = jj; a.z = tt; a.w = nn;
                    *(LA u32x4_t*)(L + p.upath + l * 32) = a;
                    *(LA uint32_t*)(L + p.upath + l * 32 + 16) = nd;
                }
                rows_e += len;
                sbP = sb; j = jj; ts = tt; plen = len; Pn = nd; leaf = lk;
                nd = lk;
            }
            pph<PROF>(pr, 2);
            if (bail) {
                if (reason == PR_ABORT) (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__));
                break;
            }
            // ---- may this element overflow its leaf?  (pipe_router's rule, on the leaf-parent's slot)
            uint32_t cl = uni(lds_ld(L, sbP + p.p_clen + j * 4)), pd = uni(lds_ld(L, sbP + p.p_pend + j * 4));
            if constexpr (PROF) wt0 = __builtin_amdgcn_s_memtime();
            if (cl + pd + 1 > bf) {
                uint32_t spins = 0;
                while (pd > 0) {
                    __builtin_amdgcn_s_sleep(1);
                    retire_poll();
                    pd = uni(lds_ld(L, sbP + p.p_pend + j * 4));
                    if (lost || ++spins > PIPE_SPIN_LIMIT) { give_up = true; PIPE_MARK(); break; }
                }
                if (give_up) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
                cl = uni(lds_ld(L, sbP + p.p_clen + j * 4));
                if (cl + 1 > bf) {
                    if (cl > bf || plen + 1 > bf || cN0 + K::nblk > cap_nodes || c32s + promos + (issued - retired) + 2 > cap32) { reason = PR_COLD; break; }
                    full = true;
                }
            }
            if constexpr (PROF) { const u64 n_ = __builtin_amdgcn_s_memtime(); rw[2] += n_ - wt0; }
            pph<PROF>(pr, 1);
            // ---- release the element to the leaf engine
            if (lane == 0) {
                LA uint32_t* pe = (LA uint32_t*)(L + sbP + p.p_pend + j * 4);
                *pe = *pe + 1u;
                u32x4_t job;
                job.x = (uint32_t)e; job.y = leaf; job.z = j | (full ? 0x80000000u : 0u); job.w = pop;
                *(LA u32x4_t*)(L + p.ring + (issued & (K::PW - 1)) * 16) = job;
                *(LA uint32_t*)(L + p.urp + (issued & (K::PW - 1)) * 4) = Pn;
            }
            issued += 1;
            PIPE_CBAR();
            lds_st(L, p.ctl + PC_HEAD * 4, issued);
            st_calls += Z + E;
            st_rows += zrows + rows_e;
            uint32_t ncommit = E;
            if (full) {
                if constexpr (PROF) wt0 = __builtin_amdgcn_s_memtime();
                uint32_t spins = 0;
                while (retired != issued) {
                    retire_poll();
                    if (lost || uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u || ++spins > PIPE_SPIN_LIMIT) { give_up = true; PIPE_MARK(); break; }
                }
                if (give_up) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
                if constexpr (PROF) { const u64 n_ = __builtin_amdgcn_s_memtime(); rw[3] += n_ - wt0; }
                if (last_ap & 1u) {
                    // appended: the leaf is split where it lies.  Every level above the leaf-parent gets the element; the
                    // leaf's own tracking row is replaced by the split (bitbirch.py:339-350) and reaches HBM without it.
                    ncommit = E - 1;
                    if (lane == 0) {
                        LA uint32_t* sp = (LA uint32_t*)(L + p.srec);
                        sp[PS_LEAF] = leaf; sp[PS_P] = Pn; sp[PS_JP] = j; sp[PS_LENP] = plen; sp[PS_TRK] = ts; sp[PS_POP] = pop; sp[PS_XOFF] = xoff;
                    }
                    reason = PR_SPLIT;
                }
            }
            // ---- commit.  Zero levels: the element's bits into the bit-sliced deferred sums
            {
                uint32_t carry = xd;
#pragma unroll
                for (int k = 0; k < PNP; ++k) {
                    const uint32_t t = dp[k] & carry;
                    dp[k] ^= carry;
                    carry = t;
                }
                used += 1;
            }
            if constexpr (PROF) levels += ncommit;
            // every exact level's tracking row (closest_subcluster.update, bitbirch.py:352-357): by the helper waves
            // (pipe_commit_try), this wave goes on
            if (lane == 0) {
                u32x2_t rq;
                rq.x = ncommit; rq.y = xoff;
                *(LA u32x2_t*)(L + p.mb + CQ_N * 4) = rq;
            }
            cposted += 1;
            cn_last = ncommit;
            cseen = 0;
            PIPE_CBAR();
            lds_st(L, p.mb + CQ_SEQ * 4, cposted);
            e += 1;
            pph<PROF>(pr, 3);
            if (reason == PR_SPLIT) break;
        }
        if constexpr (PROF) pr.ph[13] += st_stale;
        // ---- end of the run: the ring drains, deferred state goes where the next reader expects it ---------------
        commit_wait_all();  // (the helper waves write their cached cluster features back when they see the end flag)
        if (lost_c) reason = PR_ABORT;
        lds_st(L, p.ctl + PC_END * 4, 1u);
        {
            uint32_t spins = 0;
            while (uni(lds_ld(L, p.ctl + PC_TAIL * 4)) != issued) {
                __builtin_amdgcn_s_sleep(1);
                if (uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) { reason = PR_ABORT; break; }
                if (++spins > PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); reason = PR_ABORT; break; }
            }
        }
        if constexpr (PROF) {
            if (T->audit != 0 && reason != PR_ABORT) {
                // run-end audit: every upper slot against HBM (the helper waves' updates are complete: commit_wait_all above)
                retire_poll();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll 1
                for (uint32_t si = 0; si < (uint32_t)NUS; ++si) {
                    const uint32_t nd_a = (uint32_t)__builtin_amdgcn_readlane((int)utag, (int)si);
                    if (nd_a == NONE) continue;
                    const uint32_t len_a = (uint32_t)__builtin_amdgcn_readlane((int)ulen, (int)si);
                    const bool leafparent = (uni(audit_ld((const uint8_t*)(T->node_hdr + uni(*(LA volatile uint32_t*)(L + p.pslot + si * p.pslot_bytes + p.p_link))) + 4)) & HW_LEAF) != 0u;
                    pipe_audit_tracking_slot<K>(L, T, p.pslot + si * p.pslot_bytes, nd_a, len_a, leafparent && reason != PR_SPLIT);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PNP; ++k) *(LA uint32_t*)(L + p.delta + k * 256 + lane * 4) = dp[k];
        pph<PROF>(pr, 4);
    } else {
        lds_st(L, p.ctl + PC_END * 4, 1u);
    }
    (void)st_stale;
    if (lane == 0) {
        LA uint32_t* ctl = (LA uint32_t*)(L + p.ctl);
        ctl[PC_REASON] = reason;
        ctl[PC_E_LO] = (uint32_t)e;
        ctl[PC_E_HI] = (uint32_t)((u64)e >> 32);
        ctl[PC_STOPCODE] = stopcode;
        ctl[PC_DCOUNT] = used;
        ctl[PC_NZ] = Z;
        LA u64* lstats = (LA u64*)(L + p.stats);
        __hip_atomic_fetch_add(lstats + 0, (u64)st_calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(lstats + 1, (u64)st_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (used > 0 && (u64)(Z + E + 1) > lstats[6]) lstats[6] = Z + E + 1;
        if constexpr (PROF) {
            atomicAdd((unsigned long long*)&T->sphase[6], (unsigned long long)fill_cycles);
            atomicAdd((unsigned long long*)&T->sphase[7], (unsigned long long)fill_count);
            atomicAdd((unsigned long long*)&T->mlprof[0], (unsigned long long)tcf_miss);
            atomicAdd((unsigned long long*)&T->mlprof[1], (unsigned long long)levels);
            for (int i = 0; i < 4; ++i) atomicAdd((unsigned long long*)&T->rprof[i], (unsigned long long)rw[i]);
            atomicAdd((unsigned long long*)&T->mlprof[2], (unsigned long long)cw_cycles);
            atomicAdd((unsigned long long*)&T->mlprof[3], (unsigned long long)cwa_cycles);
            atomicAdd((unsigned long long*)&T->mlprof[4], (unsigned long long)fprof[0]);
            atomicAdd((unsigned long long*)&T->mlprof[5], (unsigned long long)fprof[1]);
        }
    }
    pph_out<PROF>(pr, T, lane);
}

// ---- wave 1: the leaf engine ------------------------------------------------------------------------------
// SH: wave 3 shares this wave's compares and fills (nodes of > 64 rows whose leaf-parent is not all-zero); a compile-time
// parameter - the two variants of the loop share little, and each is shorter and needs fewer live scalars without the other
template <class K, bool PROF, bool SH>
__device__ __forceinline__ void pipe_leaf(LA unsigned char* L, TreeDev* T) {
    PProf pr;
    pph_init<PROF>(pr);
    constexpr PSmem p = K::p;
    constexpr uint32_t rows = K::rows;
    constexpr int RPL = K::RPL, NL = p.nl;
    const uint32_t lane = (uint32_t)ftid() & 63u;
    uint8_t* const g_cent = T->node_cent;
    uint32_t* const g_card = T->node_card;
    uint32_t* const g_link = T->node_link;
    RowMeta* const g_rm = T->node_rm;
    NodeHdr* const g_hdr = T->node_hdr;
    uint8_t* const g_cf8 = T->cf8;
    uint32_t* const out_leaf = T->out_leaf;
    const bool have_out = out_leaf != nullptr;
    const double thr = T->thr;
    const double tolerance = T->tolerance;
    const double* const tol = T->tol_table;
    const int tol_len = (int)uni((uint32_t)T->tol_len);
    constexpr int crit = K::CRIT;
    LA uint32_t* lctr = (LA uint32_t*)(L + p.ctr);
    uint32_t cI = uni(lctr[C_IDS]), c8 = uni(lctr[C_N8]), c16 = uni(lctr[C_N16]), c32 = uni(lctr[C_N32]);
    uint32_t st_merge = 0, st_append = 0, st_calls = 0, st_rows = 0, st_stale = 0;
    // which leaf sits in which slot, and its length: lane s of two vector registers (as scalars they were a dozen of the
    // loop's live SGPRs, and the compiler parked other scalars in vector lanes around them)
    uint32_t tagv = NONE, slenv = 0;
    constexpr int NCF = p.ncf;
    uint32_t ctagv = NONE;  // tags of the cluster-feature cache: lane c
    uint32_t cvict = 0;
    uint32_t victim = 0;
    uint32_t j = 0;
    uint32_t hseq = 0;
    constexpr uint32_t MB = p.mb + 32, PART = p.part + (uint32_t)(RPL * 256), ABO = p.ctl + PC_ABORT * 4;
    bool helper_lost = false;
    u64 det[6] = {0, 0, 0, 0, 0, 0};  // (phase-timer builds) leaf compares by kind: cycles, count
    (void)det;
    constexpr bool shared = SH;
    static_assert(!SH || RPL > 1, "sharing is for nodes of several rows per lane");
    // nodes of one row per lane behind the single-level router, where this wave is the longest chain: the control block in one
    // read per poll, the packed merge path four bytes at a time (see the head of the loop body / the packed merge path)
    constexpr bool BYTES4 = RPL == 1 && !K::ML, POLL4 = RPL == 1 && !K::ML;
    // (phase-timer builds) jobs by kind - singleton target, uint8 cluster features from the LDS cache, from HBM, wide tier - and the
    // cycles between the issue of the HBM load and its data
    u64 lp[5] = {0, 0, 0, 0, 0};
    (void)lp;
    constexpr uint32_t LANES4 = (uint32_t)RPL * 256;
    // row versions, published slot tags / lengths and stamps start from zero, then wave 3 may go
#pragma unroll
    for (int sl = 0; sl < NL; ++sl)
#pragma unroll
        for (int q = 0; q < RPL; ++q) *(LA uint32_t*)(L + p.lver + (uint32_t)sl * LANES4 + ((uint32_t)q * 64 + lane) * 4) = 0u;
    if (lane < 4) *(LA uint32_t*)(L + p.pst + (8 + lane) * 4) = 0u;
    if (lane < 8) { *(LA uint32_t*)(L + p.pst + (16 + lane) * 4) = NONE; *(LA uint32_t*)(L + p.pst + (24 + lane) * 4) = 0u; }
    if constexpr (RPL > 1) { if (lane < (uint32_t)NL) *(LA uint32_t*)(L + p.llog + lane * 64) = 0u; }
    PIPE_CBAR();
    lds_st(L, p.ctl + PC_LGO * 4, 1u);
    (void)tolerance;
    // Nodes of one row per lane: row versions come from the job number - this wave is their only writer, and a version only has to
    // be odd while the row is written and afterwards an even value the row has not had before in this run: 4 j + 2 for all rows
    // after a slot fill by job j, 4 j + 4 for the row job j writes, the odd values below them meanwhile (a run takes < 2^PNP
    // jobs; pipe_pre / pipe_choose compare 20 bits).  Read back from LDS, the old version was a round trip per element.
    constexpr bool LVER = RPL == 1;
#pragma unroll 1
    while (true) {
        // ---- the next routed element -----------------------------------------------------------------------
        {
            uint32_t spins = 0;
            bool stop = false;
            while (true) {
                uint32_t h, c_end = 0, c_abort = 0;
                if constexpr (POLL4) {
                    // {head, tail, end, abort} in one read, as the router's loop top does (three dependent reads before)
                    const u32x4_t c4 = lds_ld4(L, p.ctl);
                    h = uni(c4.x); c_end = uni(c4.z); c_abort = uni(c4.w);
                } else {
                    h = uni(lds_ld(L, p.ctl + PC_HEAD * 4));
                }
                if (h != j) {
                    PIPE_CBAR();
                    break;
                }
                if constexpr (!POLL4) c_end = uni(lds_ld(L, p.ctl + PC_END * 4));
                if (c_end != 0u) {
                    // (the head is written before the end flag: read again behind the flag, it is final)
                    if (uni(lds_ld(L, p.ctl + PC_HEAD * 4)) == j) { stop = true; break; }
                    continue;
                }
                if constexpr (!POLL4) c_abort = uni(lds_ld(L, p.ctl + PC_ABORT * 4));
                if (c_abort != 0u) { stop = true; break; }
                __builtin_amdgcn_s_sleep(1);
                if (++spins > PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); stop = true; break; }
            }
            if (stop) break;
        }
        pph<PROF>(pr, 5);
        const u32x4_t job = *(LA u32x4_t*)(L + p.ring + (j & (K::PW - 1)) * 16);
        const uint32_t e = uni(job.x), leaf = uni(job.y), pop = uni(job.w);
        const bool fulljob = (uni(job.z) >> 31) != 0;
        const uint32_t xoff = p.xq + (j & (K::PW - 1)) * 256;
        const uint32_t xd = *(LA uint32_t*)(L + xoff + lane * 4);
        // ---- the leaf's slot ---------------------------------------------------------------------------------
        uint32_t si = NONE;
        {
            const u64 m = __ballot(lane < (uint32_t)NL && tagv == leaf);
            if (m != 0ull) si = (uint32_t)(__ffsll((long long)m) - 1);
        }
        bool filled = false;
        if (si == NONE) {
            si = victim;
            victim = victim + 1 == (uint32_t)NL ? 0u : victim + 1;
            const uint32_t sb = si == 0 ? p.leaf0 : p.lrest + (si - 1) * p.lslot_bytes;
            const size_t lm = (size_t)leaf * NG;
            const uint32_t hl = ldg<uint32_t>(g_hdr + leaf);
            uint32_t fv[RPL];
            // the slot changes hands: no tag while it is filled, every row's version odd, then a new even value
            if (lane == 0) lds_st(L, p.pst + (16 + si) * 4, NONE);
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                if constexpr (LVER) fv[q] = 4u * j + 1u;
                else fv[q] = lds_ld(L, p.lver + si * LANES4 + ((uint32_t)q * 64 + lane) * 4) | 1u;
                lds_st(L, p.lver + si * LANES4 + ((uint32_t)q * 64 + lane) * 4, fv[q]);
            }
            PIPE_CBAR();
            // (the helper reads what this wave wrote through when the leaf last sat in a slot: those stores have to be done)
            // (bringing in only the rows the leaf can have - the router knows an upper bound - was tried: run-time chunk
            // bounds cost the fill more than the 25 % of the bytes they save)
            if (shared) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                pipe_post(L, MB, hseq, PO_FILL, sb, leaf, 0);
                pipe_fill_rows<K, 0, PFill<K>::MID>(L, sb, g_cent, leaf);
            } else {
                pipe_fill_rows<K, 0, PFill<K>::NIT>(L, sb, g_cent, leaf);
            }
            constexpr int RMP = (int)rows * 2, RIT = (RMP + 63) / 64;
#pragma unroll
            for (int u = 0; u < RIT; ++u) {
                const uint32_t i0 = (uint32_t)u * 64 + lane;
                const uint32_t i = i0 < (uint32_t)RMP ? i0 : (uint32_t)RMP - 1;
                const u32x4_t m = ldg<u32x4_t>((const uint8_t*)(g_rm + lm) + (size_t)i * 16);
                *(LA u32x4_t*)(L + sb + p.s_rm + i * 16) = m;
            }
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const uint32_t r = (uint32_t)q * 64 + lane;
                const uint32_t rc = r < rows ? r : rows - 1;
                *(LA uint32_t*)(L + sb + p.s_card + rc * 4) = ldg<uint32_t>(g_card + lm + rc);
                *(LA uint32_t*)(L + sb + p.s_link + rc * 4) = ldg<uint32_t>(g_link + lm + rc);
            }
            const uint32_t hlen = uni(hl);
            tagv = lane == si ? leaf : tagv;
            slenv = lane == si ? hlen : slenv;
            if (shared && !pipe_wait_helper(L, MB, hseq, ABO)) { helper_lost = true; break; }
            PIPE_CBAR();
#pragma unroll
            for (int q = 0; q < RPL; ++q) lds_st(L, p.lver + si * LANES4 + ((uint32_t)q * 64 + lane) * 4, fv[q] + 1u);
            if (lane == 0) {
                // (what was pre-compared against the slot's previous rows is out of the log's reach)
                if constexpr (RPL > 1) lds_st(L, p.llog + si * 64, lds_ld(L, p.llog + si * 64) + PLOGK + 1);
                lds_st(L, p.pst + (24 + si) * 4, hlen);
                PIPE_CBAR();
                lds_st(L, p.pst + (16 + si) * 4, leaf);
            }
            filled = true;
            (void)filled;
            pph<PROF>(pr, 6);
        }
        const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)slenv, (int)si);
        const uint32_t sb = si == 0 ? p.leaf0 : p.lrest + (si - 1) * p.lslot_bytes;
        // ---- closest BitFeature of the leaf, merge test (bitbirch.py:317-336, _merges.py) --------------------------
        uint32_t jl = 0, inter = 0;
        int cls = 1;
        // row changes of the slot so far (this wave is the only writer; kept for nodes of several rows per lane only, see pipe_prel_try)
        constexpr bool CHLOG = RPL > 1 && !SH;
        uint32_t cnow = 0;
        if constexpr (!CHLOG) {
            bool pre = false;
            if (!shared) {
                const uint32_t stp = uni(lds_ld(L, p.pst + (8 + (j & (K::PREWL - 1))) * 4));
                pre = stp == ((j + 1) | (si << 28));
                PIPE_CBAR();
            }
            if (pre) {
                pipe_choose<RPL>(L, sb, sb + p.s_card, len, pop, xd, p.preL + (j & (K::PREWL - 1)) * LANES4, p.lver + si * LANES4, jl, inter, st_stale);
                if constexpr (PROF) { pr.ph[14] += 1; cls = 2; }
            } else {
                if (!pipe_compare<RPL>(L, MB, PART, ABO, hseq, sb, sb + p.s_card, len, xoff, pop, jl, inter, shared)) { helper_lost = true; break; }
            }
        } else {
            bool pre = false;
            cnow = uni(lds_ld(L, p.llog + si * 64));
            u32x4_t rec = (u32x4_t)(0);
            if (!shared && !filled) {
                const uint32_t stp = uni(lds_ld(L, p.pst + (8 + (j & (K::PREWL - 1))) * 4));
                rec = *(LA volatile u32x4_t*)(L + p.prec + (j & (K::PREWL - 1)) * 16);  // (written before the stamp, read behind it)
                pre = stp == ((j + 1) | (si << 28));
                PIPE_CBAR();
            }
            bool chosen = false;
            if (pre) {
                // The helper's first-argmax stands for every row that has not changed since its change count c1; the rows of
                // the changes since are in the slot's log: their current keys are folded in (np.argmax: the highest key, the
                // lowest row among equals).  If the helper's best row is among them and its key went down, the others' order
                // is unknown: the long way.
                const uint32_t c1 = uni(rec.x), brow0 = uni(rec.y);
                const uint32_t delta = cnow - c1;
                if (delta <= PLOGK && brow0 != NONE) {
                    const uint32_t bkey0 = uni(rec.w), binter0 = uni(rec.z);
                    if (delta == 0) {
                        jl = brow0; inter = binter0; chosen = true; cls = 0;
                    } else {
                        // all changed rows at once: eight lanes per change.  Lane (8 g + s) takes 32 bytes of the row of change
                        // c1 + 1 + g; three adds across the eight lanes make the row's intersection, every lane forms the key.
                        const uint32_t g = lane >> 3, sub = lane & 7u;
                        const bool live = g < delta;
                        const uint32_t r = lds_ld(L, p.llog + si * 64 + 4 + ((c1 + 1u + (live ? g : 0u)) & (PLOGK - 1)) * 4);
                        const u32x4_t ra = *(LA u32x4_t*)(L + sb + __umul24(r, FRBS) + sub * 32);
                        const u32x4_t rb = *(LA u32x4_t*)(L + sb + __umul24(r, FRBS) + sub * 32 + 16);
                        const u32x4_t xa = *(LA u32x4_t*)(L + xoff + sub * 32);
                        const u32x4_t xb = *(LA u32x4_t*)(L + xoff + sub * 32 + 16);
                        const uint32_t cd = *(LA uint32_t*)(L + sb + p.s_card + r * 4);
                        uint32_t val = popc4v_acc(rb & xb, popc4v_acc(ra & xa, 0u));
                        val += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)val, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
                        val += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)val, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
                        val += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)val, 0x141, 0xF, 0xF, false);  // row_half_mirror
                        uint32_t un = cd + pop - val;
                        un = un < 1u ? 1u : un;
                        const uint32_t key = live ? sim_key(val, un) : 0u;
                        // (the helper's best row itself: as long as its key has not gone down it still is ahead of every row
                        // that has not changed - lower ones, and equal ones behind it)
                        const bool down = __ballot(live && r == brow0 && key < bkey0) != 0ull;
                        if (!down) {
                            const uint32_t kmax = wmax32(key);
                            const uint32_t rmin = wmin32(live && key == kmax ? r : NONE);
                            const u64 mm = __ballot(live && key == kmax && r == rmin);
                            const uint32_t vmax = rdlane(val, __ffsll((long long)mm) - 1);
                            // np.argmax over the changed rows and the helper's maximum: the highest key, the lowest row among
                            // equals (a changed row's current value replaces the helper's value of the same row)
                            if (kmax > bkey0 || (kmax == bkey0 && rmin <= brow0)) { jl = rmin; inter = vmax; }
                            else { jl = brow0; inter = binter0; }
                            chosen = true; cls = 0;
                            st_stale += delta;
                        }
                    }
                }
                if constexpr (PROF) pr.ph[14] += 1;
            }
            if (!chosen) {
                if (pre) {
                    pipe_choose<RPL>(L, sb, sb + p.s_card, len, pop, xd, p.preL + (j & (K::PREWL - 1)) * LANES4, p.lver + si * LANES4, jl, inter, st_stale);
                    cls = 2;
                } else {
                    if (!pipe_compare<RPL>(L, MB, PART, ABO, hseq, sb, sb + p.s_card, len, xoff, pop, jl, inter, shared)) { helper_lost = true; break; }
                }
            }
        }
        st_calls += 1;
        st_rows += len;
        if constexpr (PROF) {
            det[2 * cls] += __builtin_amdgcn_s_memtime() - pr.mark;
            det[2 * cls + 1] += 1;
        }
        pph<PROF>(pr, 7);
        const u32x4_t ma = *(LA u32x4_t*)(L + sb + p.s_rm + jl * 32);
        const u32x4_t mb = *(LA u32x4_t*)(L + sb + p.s_rm + jl * 32 + 16);
        const uint32_t Tsub = uni(ma.x), nT = uni(ma.y), slotT = uni(ma.z);
        const u64 s1T = ((u64)uni(mb.y) << 32) | uni(mb.x);
        const u64 s2T = ((u64)uni(mb.w) << 32) | uni(mb.z);
        const uint32_t tierT = slotT >> 30;
        const u64 new_n = (u64)nT + 1;
        const size_t lm = (size_t)leaf * NG;
        // the element's bits as one byte per feature (0 / 1), four features per dword, in the order of the uint8 cluster
        // features: bit-reversed, feature 8 b + q of the lane's dword sits at bit 24 - 8 b + q, and four adjacent bits
        // are spread to four bytes by one 24-bit multiply
        const uint32_t xr = __builtin_bitreverse32(xd);
        uint32_t xs[8];
        if constexpr (!BYTES4) {  // (BYTES4: spread where the decision is known to need them, see below)
#pragma unroll
            for (int u = 0; u < 8; ++u) xs[u] = __umul24((xr >> (24 - 8 * (u >> 1) + 4 * (u & 1))) & 15u, 0x204081u) & 0x01010101u;
        }
        const bool packed = tierT == 0 && new_n <= 255;  // uint8 cluster features before and after: the common case
        const u64 s1n = s1T + pop;
        // merge_accept_fn on exact moments (_merges.py), float64 in the reference's operation order
        auto decide = [&](u64 dot) -> bool {
            const u64 s2n = s2T + 2ull * dot + pop;
            bool acc = false;
            if constexpr (crit == BBH_CRIT_DIAMETER) {
                // jt_isim_from_sum(new_ls, new_n) >= threshold (_merges.py:56-69).  The quotient a / d is only formed when
                // a is within 2^-48 of threshold * d: outside that band the correctly rounded quotient is on the same side
                // of the threshold as the exact one (similarity.cpp:297-300 operation order for a and d).
                // tests/test_hip_tree_thresholds.py walks a ladder of thresholds through this band (0, +-1, +-8, +-24, +-40,
                // +-1000 ulps around quotients that thousands of merges hit exactly) against the oracle.
                if (s1n == 0ull) {
                    acc = 1.0 >= thr;
                } else {
                    const double a = (double)(s2n - s1n) / 2.0;
                    const double d = (a + (double)(new_n * s1n)) - (double)s2n;
                    const double t = thr * d;
                    if (d > 0.0 && a >= t * (1.0 + 0x1p-48)) acc = true;
                    else if (d > 0.0 && a <= t * (1.0 - 0x1p-48)) acc = false;
                    else acc = a / d >= thr;
                }
            } else if constexpr (crit == BBH_CRIT_TOL_DIAMETER) {
                const double new_dc = isim_from_moments(s1n, s2n, new_n);
                if (new_dc < thr) acc = false;
                else if (nT == 1) acc = true;
                else {
                    double told = 0.0;
                    if (tol != nullptr && nT < (uint32_t)tol_len) {
                        typedef const double __attribute__((address_space(4))) cdouble_t;
                        told = *((cdouble_t*)(uintptr_t)tol + nT);
                    }
                    acc = new_dc >= isim_from_moments(s1T, s2T, nT) - told;
                }
            }
            return uni((uint32_t)acc) != 0;
        };
        if constexpr (K::ML) {
            // Watermark for the multi-level router: every global store of the jobs before this one has completed (they were
            // issued a leaf compare ago: the wait is short), so what it reads from HBM is at least that recent.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            lds_st(L, p.ctl + PC_WM * 4, j);
        }
        bool accept;
        u64 s2n = 0;
        uint32_t cw = 0, slotN = slotT, out_id, resw = 0;
        // (the two variants share no register arrays: an array that is live across their join costs a copy per element
        // on every control-flow edge around it)
        if (packed) {
            uint32_t w[8];
            uint32_t chit = NONE;  // entry of the cluster-feature cache that holds this BitFeature's linear sum
            u64 dot;
            if (nT == 1) {
                // a singleton: its linear sum is its centroid (bitbirch.py:423-435; it has no uint8 slot yet, see SLOT_LAZY8),
                // the dot product the intersection
                if constexpr (!BYTES4) {
                    const uint32_t cr = __builtin_bitreverse32(*(LA uint32_t*)(L + sb + __umul24(jl, FRBS) + lane * 4));
#pragma unroll
                    for (int u = 0; u < 8; ++u) w[u] = __umul24((cr >> (24 - 8 * (u >> 1) + 4 * (u & 1))) & 15u, 0x204081u) & 0x01010101u;
                }
                // (BYTES4: the two rows are spread to bytes once the pair is accepted - a rejected pair never needs them)
                dot = inter;
                if constexpr (PROF) lp[0] += 1;
            } else {
                if constexpr (NCF > 0) {
                    const u64 m = __ballot(lane < (uint32_t)NCF && ctagv == slotT);
                    if (m != 0ull) chit = (uint32_t)(__ffsll((long long)m) - 1);
                }
                u32x4_t q0, q1;
                if (chit != NONE) {
                    q0 = *(LA u32x4_t*)(L + p.cfc + chit * 2048 + lane * 32);
                    q1 = *(LA u32x4_t*)(L + p.cfc + chit * 2048 + lane * 32 + 16);
                    if constexpr (PROF) lp[1] += 1;
                } else {
                    const size_t cfi = (size_t)slotT * 2048 + (size_t)lane * 32;
                    q0 = ldg<u32x4_t>(g_cf8 + cfi);
                    q1 = ldg<u32x4_t>(g_cf8 + cfi + 16);
                    if constexpr (PROF) {
                        // (every store of the jobs before was issued a compare ago: what is waited for here is this load)
                        const u64 w0 = __builtin_amdgcn_s_memtime();
                        asm volatile("s_waitcnt vmcnt(0)" : "+v"(q0), "+v"(q1) : : "memory");
                        lp[4] += __builtin_amdgcn_s_memtime() - w0;
                        lp[2] += 1;
                    }
                }
                w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w; w[4] = q1.x; w[5] = q1.y; w[6] = q1.z; w[7] = q1.w;
                uint32_t d32 = 0;
                if constexpr (BYTES4) {
                    // one 4 x u8 dot-accumulate per dword on the element's 0 / 1 bytes
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        xs[u] = bbp_expand_dword(xr, u);
                        d32 = __builtin_amdgcn_udot4(w[u], xs[u], d32, false);
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < 8; ++u) d32 = __builtin_amdgcn_sad_u8(w[u] & ((xs[u] << 8) - xs[u]), 0u, d32);  // (0x01 -> 0xFF per byte)
                }
                dot = wsum32(d32);
            }
            pph<PROF>(pr, 8);
            s2n = s2T + 2ull * dot + pop;
            accept = decide(dot);
            if (accept) {
                // replace_n_samples_and_linear_sum (bitbirch.py:476-484), same tier, same slot
                if (nT == 1) {
                    // two members: a feature is in the centroid if either has it (2 ls >= 2), no majority vote to take;
                    // the BitFeature gets its uint8 row now (SLOT_LAZY8)
                    slotN = c8++;
                    if constexpr (BYTES4) {
                        const uint32_t cd = *(LA uint32_t*)(L + sb + __umul24(jl, FRBS) + lane * 4);
                        const uint32_t cr = __builtin_bitreverse32(cd);
#pragma unroll
                        for (int u = 0; u < 8; ++u) w[u] = bbp_expand_dword(cr, u) + bbp_expand_dword(xr, u);
                        cw = cd | xd;
                    } else {
#pragma unroll
                        for (int u = 0; u < 8; ++u) w[u] += xs[u];
                        cw = *(LA uint32_t*)(L + sb + __umul24(jl, FRBS) + lane * 4) | xd;
                    }
                } else if constexpr (BYTES4) {
                    // the majority vote four bytes at a time (bb_pipe_bytes.h); bytes stay below 256: new_n <= 255
#pragma unroll
                    for (int u = 0; u < 8; ++u) w[u] += xs[u];
                    cw = bbp_centroid_dword8(w, ((uint32_t)new_n + 1u) >> 1);
                } else {
                    const uint32_t hm1 = (((uint32_t)new_n + 1u) >> 1) - 1u;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        uint32_t byte = 0;
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const int u = 2 * b + (q >> 2), k = q & 3;
                            if (k == 0) w[u] += xs[u];  // bytes stay below 256: new_n <= 255
                            byte = __builtin_amdgcn_alignbit(byte, hm1 - ((w[u] >> (8 * k)) & 0xFFu), 31);
                        }
                        cw |= (byte & 0xFFu) << (8 * b);
                    }
                }
                u32x4_t q0, q1;
                q0.x = w[0]; q0.y = w[1]; q0.z = w[2]; q0.w = w[3];
                q1.x = w[4]; q1.y = w[5]; q1.z = w[6]; q1.w = w[7];
                const size_t cfo = (size_t)slotN * 2048 + (size_t)lane * 32;
                stg<u32x4_t>(g_cf8 + cfo, q0);
                stg<u32x4_t>(g_cf8 + cfo + 16, q1);
                if constexpr (NCF > 0) {
                    if (chit == NONE) {  // first in, first out
                        chit = cvict;
                        cvict = cvict + 1 == (uint32_t)NCF ? 0u : cvict + 1;
                        ctagv = lane == chit ? slotN : ctagv;
                    }
                    *(LA u32x4_t*)(L + p.cfc + chit * 2048 + lane * 32) = q0;
                    *(LA u32x4_t*)(L + p.cfc + chit * 2048 + lane * 32 + 16) = q1;
                }
            }
        } else {
            // uint16 / uint32 cluster features, and the insertion that moves a BitFeature up a tier (256 / 65536 members)
            uint32_t v[32];
            uint16_t* const g_cf16 = T->cf16;
            uint32_t* const g_cf32 = T->cf32;
            const size_t cfi = (size_t)(slotT & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
            if (tierT == 0) {
                const u32x4_t q0 = ldg<u32x4_t>(g_cf8 + cfi), q1 = ldg<u32x4_t>(g_cf8 + cfi + 16);
                const uint32_t ww[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
                for (int i = 0; i < 32; ++i) v[i] = (ww[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            } else if (tierT == 1) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const u32x4_t q = ldg<u32x4_t>(g_cf16 + cfi + u * 8);
                    v[8 * u] = q.x & 0xFFFFu; v[8 * u + 1] = q.x >> 16; v[8 * u + 2] = q.y & 0xFFFFu; v[8 * u + 3] = q.y >> 16;
                    v[8 * u + 4] = q.z & 0xFFFFu; v[8 * u + 5] = q.z >> 16; v[8 * u + 6] = q.w & 0xFFFFu; v[8 * u + 7] = q.w >> 16;
                }
            } else {
                cf32_lane_load(g_cf32, slotT, lane, v);
            }
            u64 d = 0;
#pragma unroll
            for (int i = 0; i < 32; ++i) d += (u64)(v[i] & (0u - xbit(xd, i)));
            const u64 dot = wsum64(d);
            if constexpr (PROF) lp[3] += 1;
            pph<PROF>(pr, 8);
            s2n = s2T + 2ull * dot + pop;
            accept = decide(dot);
            if (accept) {
                if (tierT == 0) {
                    ctagv = ctagv == slotT ? NONE : ctagv;  // leaves the uint8 tier
                }
#pragma unroll
                for (int i = 0; i < 32; ++i) v[i] += xbit(xd, i);
                cw = centroid_dword31(v, (uint32_t)new_n);
                const uint32_t ntier = tier_for(new_n) > tierT ? tier_for(new_n) : tierT;
                if (ntier != tierT) {
                    slotN = (ntier << 30) | (ntier == 1 ? c16++ : c32++);
                    resw |= 2u;
                }
                const size_t cfo = (size_t)(slotN & 0x3FFFFFFFu) * 2048 + (size_t)lane * 32;
                if (ntier == 1) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        u32x4_t q;
                        q.x = v[8 * u] | (v[8 * u + 1] << 16); q.y = v[8 * u + 2] | (v[8 * u + 3] << 16);
                        q.z = v[8 * u + 4] | (v[8 * u + 5] << 16); q.w = v[8 * u + 6] | (v[8 * u + 7] << 16);
                        stg<u32x4_t>(g_cf16 + cfo + u * 8, q);
                    }
                } else {
                    cf32_lane_store(g_cf32, slotN, lane, v);
                }
            }
        }
        if (accept) {
            const uint32_t cardn = wsum32((uint32_t)__popc(cw));
            uint32_t rv;
            if constexpr (LVER) rv = 4u * j + 2u;
            else rv = uni(lds_ld(L, p.lver + si * LANES4 + jl * 4));
            if (lane == 0) lds_st(L, p.lver + si * LANES4 + jl * 4, rv + 1);
            PIPE_CBAR();
            *(LA uint32_t*)(L + sb + __umul24(jl, FRBS) + lane * 4) = cw;
            if constexpr (CHLOG) {
                // (the row's popcount belongs to the row: inside the version window; then the change is logged and counted)
                if (lane == 0) {
                    *(LA uint32_t*)(L + sb + p.s_card + jl * 4) = cardn;
                    PIPE_CBAR();
                    lds_st(L, p.lver + si * LANES4 + jl * 4, rv + 2);
                    lds_st(L, p.llog + si * 64 + 4 + ((cnow + 1) & (PLOGK - 1)) * 4, jl);
                    PIPE_CBAR();
                    lds_st(L, p.llog + si * 64, cnow + 1);
                }
            } else {
                PIPE_CBAR();
                if (lane == 0) lds_st(L, p.lver + si * LANES4 + jl * 4, rv + 2);
            }
            stg<uint32_t>(g_cent + (lm + jl) * 256 + lane * 4, cw);
            if (lane == 0) {
                u32x4_t a, b;
                a.x = Tsub; a.y = (uint32_t)new_n; a.z = slotN; a.w = 0;
                b.x = (uint32_t)s1n; b.y = (uint32_t)(s1n >> 32); b.z = (uint32_t)s2n; b.w = (uint32_t)(s2n >> 32);
                stg<u32x4_t>((uint8_t*)(g_rm + lm + jl), a);
                stg<u32x4_t>((uint8_t*)(g_rm + lm + jl) + 16, b);
                stg<uint32_t>(g_card + lm + jl, cardn);
                *(LA u32x4_t*)(L + sb + p.s_rm + jl * 32) = a;
                *(LA u32x4_t*)(L + sb + p.s_rm + jl * 32 + 16) = b;
                *(LA uint32_t*)(L + sb + p.s_card + jl * 4) = cardn;
                if (slotN != slotT) {
                    stg<uint32_t>(g_link + lm + jl, slotN);
                    *(LA uint32_t*)(L + sb + p.s_link + jl * 4) = slotN;
                }
            }
            st_merge += 1;
            out_id = Tsub;
        } else {
            // append_subcluster (bitbirch.py:284-287): a new leaf BitFeature in the next row (the router made sure it fits)
            const uint32_t s = cI++;
            const uint32_t slotw = SLOT_LAZY8;  // no uint8 slot: one fingerprint's cluster features are its centroid row
            const size_t m = lm + len;
            uint32_t rv;
            if constexpr (LVER) rv = 4u * j + 2u;
            else rv = uni(lds_ld(L, p.lver + si * LANES4 + len * 4));
            if (lane == 0) lds_st(L, p.lver + si * LANES4 + len * 4, rv + 1);
            PIPE_CBAR();
            *(LA uint32_t*)(L + sb + __umul24(len, FRBS) + lane * 4) = xd;
            if constexpr (CHLOG) {
                if (lane == 0) {
                    *(LA uint32_t*)(L + sb + p.s_card + len * 4) = pop;
                    PIPE_CBAR();
                    lds_st(L, p.lver + si * LANES4 + len * 4, rv + 2);
                    lds_st(L, p.pst + (24 + si) * 4, len + 1);
                    lds_st(L, p.llog + si * 64 + 4 + ((cnow + 1) & (PLOGK - 1)) * 4, len);
                    PIPE_CBAR();
                    lds_st(L, p.llog + si * 64, cnow + 1);
                }
            } else {
                PIPE_CBAR();
                if (lane == 0) {
                    lds_st(L, p.lver + si * LANES4 + len * 4, rv + 2);
                    lds_st(L, p.pst + (24 + si) * 4, len + 1);
                }
            }
            stg<uint32_t>(g_cent + m * 256 + lane * 4, xd);
            if (lane == 0) {
                u32x4_t a, b;
                a.x = s; a.y = 1u; a.z = slotw; a.w = 0;
                b.x = pop; b.y = 0; b.z = pop; b.w = 0;
                stg<u32x4_t>((uint8_t*)(g_rm + m), a);
                stg<u32x4_t>((uint8_t*)(g_rm + m) + 16, b);
                stg<uint32_t>(g_card + m, pop);
                stg<uint32_t>(g_link + m, slotw);
                stg<uint32_t>(g_hdr + leaf, len + 1);
                *(LA u32x4_t*)(L + sb + p.s_rm + len * 32) = a;
                *(LA u32x4_t*)(L + sb + p.s_rm + len * 32 + 16) = b;
                *(LA uint32_t*)(L + sb + p.s_card + len * 4) = pop;
                *(LA uint32_t*)(L + sb + p.s_link + len * 4) = slotw;
            }
            slenv = lane == si ? len + 1 : slenv;
            st_append += 1;
            out_id = s;
            resw |= 1u;
        }
        if (lane == 0 && have_out) stg<uint32_t>(out_leaf + e, out_id);
        if (fulljob && lane == 0) ((LA uint32_t*)(L + p.srec))[PS_SI] = si;
        if constexpr (K::ML) resw |= (len + (resw & 1u)) << 8;  // the leaf's length after this job
        lds_st(L, p.res + (j & (K::PW - 1)) * 4, resw);
        j += 1;
        PIPE_CBAR();
        lds_st(L, p.ctl + PC_TAIL * 4, j);
        pph<PROF>(pr, 9);
    }
    pph<PROF>(pr, 5);
    if constexpr (PROF) {
        pr.ph[15] += st_stale;
        if (lane == 0)
            for (int i = 0; i < 6; ++i) atomicAdd((unsigned long long*)&T->sphase[i], (unsigned long long)det[i]);
        if (lane == 0)
            for (int i = 0; i < 5; ++i) atomicAdd((unsigned long long*)&T->lprof[i], (unsigned long long)lp[i]);
    }
    pph_out<PROF>(pr, T, lane);
    (void)helper_lost;
    if constexpr (PROF) {
        if (T->audit != 0 && !helper_lost && uni(lds_ld(L, p.ctl + PC_ABORT * 4)) == 0u) {
            // run-end audit: every leaf this wave holds in a slot against HBM - rows, popcounts, row records, length
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll 1
            for (uint32_t si = 0; si < (uint32_t)NL; ++si) {
                const uint32_t lf = (uint32_t)__builtin_amdgcn_readlane((int)tagv, (int)si);
                if (lf == NONE) continue;
                const uint32_t len_a = (uint32_t)__builtin_amdgcn_readlane((int)slenv, (int)si);
                const uint32_t sb_a = si == 0 ? p.leaf0 : p.lrest + (si - 1) * p.lslot_bytes;
                if (lane == 0) atomicAdd(&g_pipe_audit_runs, 1ull);
                if (uni(audit_ld(g_hdr + lf)) != len_a) { PIPE_AUDIT_FAIL(10); break; }
                pipe_audit_rows<K>(L, T->node_cent, sb_a, lf, len_a, 7);
#pragma unroll 1
                for (int q = 0; q < RPL; ++q) {
                    const uint32_t r = (uint32_t)q * 64 + lane;
                    const bool in = r < len_a;
                    const uint32_t rc = in ? r : 0u;
                    const size_t m = (size_t)lf * NG + rc;
                    if (__ballot(in && *(LA volatile uint32_t*)(L + sb_a + p.s_card + rc * 4) != audit_ld(T->node_card + m)) != 0ull) { PIPE_AUDIT_FAIL(8); break; }
                    bool bad = false;
                    for (int w = 0; w < 8; ++w)
                        bad = bad || (w != 3 && *(LA volatile uint32_t*)(L + sb_a + p.s_rm + rc * 32 + w * 4) != audit_ld((const uint8_t*)(g_rm + m) + w * 4));
                    if (__ballot(in && bad) != 0ull) { PIPE_AUDIT_FAIL(9); break; }
                }
            }
        }
    }
    if constexpr (SH) pipe_post(L, MB, hseq, PO_EXIT, 0, 0, 0);  // (wave 3 in its sharing role)
    if (lane == 0) {
        lctr[C_IDS] = cI; lctr[C_N8] = c8; lctr[C_N16] = c16; lctr[C_N32] = c32;
        LA u64* lstats = (LA u64*)(L + p.stats);
        __hip_atomic_fetch_add(lstats + 0, (u64)st_calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(lstats + 1, (u64)st_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(lstats + 2, (u64)st_merge, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(lstats + 3, (u64)st_append, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// ---- between runs, all four waves: the deferred zero-level sums go into the tracking rows' cluster features ------
template <class K>
__device__ __forceinline__ void pipe_flush_delta(LA unsigned char* L, TreeDev* T) {
    constexpr PSmem p = K::p;
    const int tid = threadIdx.x;
    LA uint32_t* ctl = (LA uint32_t*)(L + p.ctl);
    const uint32_t cnt = uni(ctl[PC_DCOUNT]), nz = uni(ctl[PC_NZ]);
    if (cnt == 0 || nz == 0) return;
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < PNP; ++k) {
        const uint32_t byte = *(LA uint8_t*)(L + p.delta + k * 256 + tid);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] |= ((byte >> (7 - q)) & 1u) << k;
    }
    uint32_t* const g_cf32 = T->cf32;
    RowMeta* const g_rm = T->node_rm;
#pragma unroll 1
    for (uint32_t z = 0; z < nz; ++z) {
        LA uint32_t* zr = (LA uint32_t*)(L + p.zrec + z * 32);
        const uint32_t nd = uni(zr[0]), ts = uni(zr[1]);
        uint32_t* cf = g_cf32 + (size_t)(ts & 0x3FFFFFFFu) * 2048 + (size_t)tid * 8;
        u32x4_t q0 = ldg<u32x4_t>(cf), q1 = ldg<u32x4_t>(cf + 4);
        q0.x += v[0]; q0.y += v[1]; q0.z += v[2]; q0.w += v[3];
        q1.x += v[4]; q1.y += v[5]; q1.z += v[6]; q1.w += v[7];
        stg<u32x4_t>(cf, q0);
        stg<u32x4_t>(cf + 4, q1);
        if (tid == 0) {
            uint8_t* rm = (uint8_t*)(g_rm + (size_t)nd * NG);
            const uint32_t n0 = ldg<uint32_t>(rm + 4);
            stg<uint32_t>(rm + 4, n0 + cnt);
            stg<uint32_t>(rm + 12, 0u);
        }
    }
}

template <class K, bool PROF>
__device__ __forceinline__ void tree_pipe_body(unsigned char* smem_raw, TreeDev* T) {
    constexpr PSmem p = K::p;
    LA unsigned char* L = (LA unsigned char*)smem_raw;
    const int tid = threadIdx.x;
    const uint32_t wave = uni((uint32_t)tid >> 6);
    LA uint32_t* lctr = (LA uint32_t*)(L + p.ctr);
    LA u64* lstats = (LA u64*)(L + p.stats);
    LA uint32_t* ctl = (LA uint32_t*)(L + p.ctl);
    if (tid < C_COUNT) lctr[tid] = T->ctr[tid];
    if (tid == 8) lctr[8] = STOP_DONE;
    if (tid < 8) lstats[tid] = T->stats[tid];
    if (tid < 16) ((LA u32x4_t*)(L + p.x))[tid] = (u32x4_t)(0);
    if (tid < PZ * 8) ((LA uint32_t*)(L + p.zrec))[tid] = NONE;
    __syncthreads();
    const long long n_elems = T->n_elems;
    long long e = 0;
    int stop = STOP_DONE;
    while (e < n_elems) {
        if (tid < 16) ctl[tid] = 0u;
        if (tid >= 16 && tid < 32) ((LA uint32_t*)(L + p.mb))[tid - 16] = 0u;
        __syncthreads();
        if (wave == 0) {
            if constexpr (K::ML) pipe_router_ml<K, PROF>(L, T, e);
            else pipe_router<K, PROF>(L, T, e);
        }
        else if (wave == 1) {
            if constexpr (K::RPL == 1) {
                pipe_leaf<K, PROF, false>(L, T);
            } else {
                // (which variant: known when the router has looked at the leaf-parent - before anything is routed)
                uint32_t spins = 0;
                bool role_known = false;
                while (!role_known) {
                    if (uni(lds_ld(L, p.ctl + PC_PGO * 4)) != 0u) role_known = true;
                    else if (uni(lds_ld(L, p.ctl + PC_END * 4)) != 0u || uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) break;
                    else if (++spins > 64u * PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); break; }
                }
                if (role_known) {
                    if (uni(lds_ld(L, p.ctl + PC_PZERO * 4)) != 0u) pipe_leaf<K, PROF, false>(L, T);
                    else pipe_leaf<K, PROF, true>(L, T);
                }
            }
        }
        else if (wave == 2) pipe_prep<K>(L, T, e);
        else if (K::ML) pipe_prel_cmt<K>(L, T);
        else if (K::RPL == 1) pipe_prel<K>(L, 0u, 1u);
        else {
            // nodes of > 64 rows: wave 3 shares the leaf engine's compares and fills - unless the leaf-parent is all-zero, when
            // wave 2 needs no time for it and the two helpers pre-compare the leaf engine's jobs alternately
            uint32_t spins = 0;
            bool role_known = false;
            while (!role_known) {
                if (uni(lds_ld(L, p.ctl + PC_PGO * 4)) != 0u) role_known = true;
                else if (uni(lds_ld(L, p.ctl + PC_END * 4)) != 0u || uni(lds_ld(L, p.ctl + PC_ABORT * 4)) != 0u) break;
                else if (++spins > 64u * PIPE_SPIN_LIMIT) { (PIPE_MARK(), lds_st(L, p.ctl + PC_ABORT * 4, (uint32_t)__LINE__)); break; }
            }
            if (role_known) {
                if (uni(lds_ld(L, p.ctl + PC_PZERO * 4)) != 0u) pipe_prel<K>(L, 1u, 2u);
                else pipe_helper<K>(L, T, 1);
            }
        }
        __syncthreads();
        const u64 c0 = PROF ? __builtin_amdgcn_s_memtime() : 0;
        const uint32_t reason = uni(ctl[PC_REASON]);
        e = (long long)(((u64)uni(ctl[PC_E_HI]) << 32) | uni(ctl[PC_E_LO]));
        pipe_flush_delta<K>(L, T);
        __syncthreads();
        const u64 c1 = PROF ? __builtin_amdgcn_s_memtime() : 0;
        if constexpr (PROF) { if (tid == 0) T->phase[10] += c1 - c0; }
        if (reason == PR_DONE) break;
        if (reason == PR_FLUSH) continue;
        if (reason == PR_SPLIT) {
            // element e - 1 was appended to a full leaf: the leaf's slot becomes slot 0 (the one the split's scratch does not
            // overlay), the element's row goes where split_node reads it, and the leaf is split in place
            LA uint32_t* sp = (LA uint32_t*)(L + p.srec);
            const uint32_t s_leaf = uni(sp[PS_LEAF]), s_P = uni(sp[PS_P]), s_jp = uni(sp[PS_JP]), s_lenP = uni(sp[PS_LENP]);
            const uint32_t s_trk = uni(sp[PS_TRK]), s_pop = uni(sp[PS_POP]), s_xoff = uni(sp[PS_XOFF]), s_si = uni(sp[PS_SI]);
            __syncthreads();
            if (s_si != 0) {
                const uint32_t src = p.lrest + (s_si - 1) * p.lslot_bytes;
                for (uint32_t i = (uint32_t)tid; i < p.lslot_bytes / 16; i += TB)
                    *(LA u32x4_t*)(L + p.leaf0 + i * 16) = *(LA u32x4_t*)(L + src + i * 16);
            }
            if (tid < 64) ((LA uint32_t*)(L + p.x))[tid] = *(LA uint32_t*)(L + s_xoff + tid * 4);
            __syncthreads();
            cold_leaf_split_p<K::BF, PROF>(smem_raw, T, e - 1, s_pop, s_leaf, s_P, s_jp, s_lenP, s_trk);
            if constexpr (PROF) { if (tid == 0) { T->phase[11] += __builtin_amdgcn_s_memtime() - c1; } }
            const uint32_t sstop = uni(lctr[8]);
            __syncthreads();
            if (sstop != STOP_DONE) { stop = (int)sstop; break; }
            continue;
        }
        if (reason == PR_STOP) { stop = (int)uni(ctl[PC_STOPCODE]); break; }
        if (reason == PR_UNSUP) { stop = STOP_PIPE_UNSUPPORTED; break; }
        if (reason == PR_NEEDML) { stop = STOP_PIPE_NEEDS_ML; break; }
        if (reason == PR_PREFSL) { stop = STOP_PIPE_PREFERS_SL; break; }
        if (reason == PR_ABORT) {
            if (tid == 0) T->giveup_line = uni(ctl[PC_ABORT]);
            stop = STOP_INTERNAL;
            break;
        }
        // PR_COLD: element e needs the complete engine (a full leaf, an unstable zero level, a huge cluster)
        if (e >= n_elems) break;
        cold_insert_one_p<K::BF>(smem_raw, T, e);
        const uint32_t cstop = uni(lctr[8]), cdone = uni(lctr[9]);
        // (the complete engine may have split a node of the zero levels: the row that tracks the split node keeps its cf32 slot
        // (split_node) with another node's sums in it - the cached flip distances, keyed by node and slot, start over)
        if (tid < PZ * 8) ((LA uint32_t*)(L + p.zrec))[tid] = NONE;
        __syncthreads();
        if constexpr (PROF) { if (tid == 0) T->phase[11] += __builtin_amdgcn_s_memtime() - c1; }
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
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_tree_pipe(TreeDev* trees) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    tree_pipe_body<K, PROF>(smem_raw, trees + blockIdx.x);
}

#endif  // __HIPCC__
