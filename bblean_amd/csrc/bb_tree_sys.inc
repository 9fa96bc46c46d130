// bb_tree_sys.inc -- ONE tree over MANY workgroups: the level-systolic insertion kernel (round 6; DESIGN.md section 6s).
//
// The reference's loop (bitbirch.py:769-787 -> _BFNode.insert_bf_subcluster :305-357) is sequential per NODE, not per tree:
// what element e + 1 sees of a node is that node's rows after element e passed it - the chosen row's `CF += x` and new
// majority centroid (:352-357) - and nothing else, unless a node below it split (:339-350).  k_tree_fast / k_tree_pipe run
// that chain on one workgroup, i.e. on 1 of 256 CUs, and a tree whose internal levels are informative (every level
// compares, every level's tracking row changes: real fingerprints) pays every level's compare + commit in series.  Here
// every node has an OWNER workgroup and elements flow down the tree through one-way rings in HBM / L2:
//
//   level 0   workgroup 0 owns the root and admits the elements in order: compare, guard, `CF += x` + new centroid on the
//             chosen tracking row, hand the element to the owner of the chosen child;
//   level l   the workgroups of level l (a disjoint set per level: S.lvl_first / S.lvl_count) own the nodes of that tree
//             level by hash of the node id and do the same for the elements their rings deliver;
//   leaves    the leaf owners do what the leaf does: compare, merge test on exact moments, merge or append
//             (bitbirch.py:321-337), `out_leaf[e]`.
//
// Exactness.  A node has exactly one producer - its parent's owner - and a ring is first-in first-out, so every node sees
// its elements in the reference's order BY CONSTRUCTION; two elements that are in flight at the same time are in different
// subtrees, whose rows are disjoint.  What couples subtrees is a split (a child's split rewrites its parent's rows), and
// that is what the GUARD is for: the owner of N hands e to child C without further ado only if C cannot overflow even if
// every element in flight below C adds a row to it (len(C) + pending(C) + 1 <= bf; len and the count of elements C has
// dealt with come from C's mailbox word, which C's owner rewrites after every element).  Otherwise it waits for the
// pending ones, and if C is FULL it hands e over ALONE: N's tracking row is not touched, N's owner waits, the levels below
// do the same wherever the next child is full, and the leaf's owner - with every node the split can reach quiesced above
// it - either merges (everyone commits on the way back up) or appends and runs the reference's split cascade
// (bitbirch.py:162-211, :289-303, :339-350, :778-782) with the complete engine's split_node on the quiesced chain, after
// which the owners reload.  Owners of one level never wait for their own level or the levels above, so the waits cannot
// form a cycle.  A root split changes the depth (= the assignment of workgroups to levels): the kernel drains and the host
// relaunches it.
//
// Memory model (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup visibility"): a node's rows,
// records and cluster features are touched by its owner only, with plain loads and stores (same CU).  What crosses
// workgroups: ring messages and mailbox words - naturally aligned 8-byte `sc1` stores / loads, complete by their own
// generation bit or counter, no flags, no fences - and the hand-over of a quiesced chain: agent-scope release fence by
// every owner before it hands an element over ALONE, acquire by the leaf owner before the cascade, release after it, and
// acquire by every owner that comes back from a split (and by whoever receives a message that carries a newer split epoch:
// the new node's owner).  A relaxed `sc1` poll can go on returning a stale line (tools/probe/oneway_stream.cpp,
// profiles/r06/oneway_stream_poll_modes.txt): every wait that finds nothing invalidates (agent-scope acquire fence) before
// it looks again - staleness of a mailbox only ever makes the guard more careful.  And that is still not enough: a waiter was
// caught re-reading a mailbox for five seconds - acquire fences and all - that a read-modify-write showed to hold the awaited
// value (profiles/r06/sys_stale_mailbox.txt: the per-XCD L2 keeps a line that `buffer_inv sc1` does not touch).  So the words
// workgroups talk through (rings, mailboxes, hand-over counters, control words) live in UNCACHED device memory
// (hipDeviceMallocUncached: every access goes to memory), every wait falls back to a read-modify-write read every few spins,
// and the two fences around a quiesced chain's hand-over are system-scope.
#if defined(__HIPCC__)

constexpr int SYS_MAXLVL = 8;            // tree levels (leaf level included) the kernel is laid out for
constexpr int SYS_MAXPROD = 64;          // workgroups per level: a consumer polls its producers with one wave-wide load
constexpr uint32_t SYS_R = 1024;         // messages a ring holds (more than the kernel ever has in flight: SysDev::qmax)
constexpr int STOP_SYS_RELAUNCH = 13;    // the root split (or the kernel was asked to yield): relaunch with the new depth
constexpr int STOP_SYS_UNSUPPORTED = 14; // a shape this kernel does not take (sealed node, root still a leaf, too deep)
enum SysCtl : int { SC_ABORT = 0, SC_STOP, SC_COMPLETED, SC_EPOCH, SC_FINISH, SC_ADMITTED, SC_WG_BUSY, SC_STALE_CTL, SC_COUNT = 16 };
constexpr uint32_t SYS_INV_EVERY = 4;  // a waiter invalidates (buffer_inv sc1) once per so many polls and sleeps between the others (16: 3-5 % faster, and the
                                        // randomised suite's failures at bf 254 double - profiles/r06/sys_stability.txt)
constexpr u64 SYS_SPIN_LIMIT = 12000000000ull;  // s_memtime ticks (~5 s) before a wait that must end gives up

struct SysDev {
    u64* rings;      // [G][SYS_MAXPROD][R][2]: consumer-major; two 8-byte halves per message
    u64* mail;       // [node]: acked (32) | len (16) | result of the last ALONE element (2)
    uint32_t* sent;  // [node]: elements its parent's owner has handed to it.  Owner-private PLAIN memory, like `acks`, `up` and `laste`: a
                     // word its writer reads back belongs with the tree data (plain loads and stores, handed from one owner to the
                     // next under the chain's fences), not with the words polled across workgroups - an owner that read its own
                     // atomic exchange back from uncached memory a step later did not always get it (bf 254 refills a node every
                     // step: counts that stood still, `acked` behind `sent` for good; profiles/r06/sys_stability.txt)
    uint32_t* acks;  // [node]: elements its owner has dealt with (the count its mailbox publishes; the owner's own copy)
    u64* up;         // [node]: (parent << 32) | row, written by the parent's owner before an ALONE hand-over
    uint32_t* laste; // [node]: 1 + the last element its owner dealt with (owner-private): elements must arrive in increasing order
    uint32_t* ctl;   // SysCtl words
    unsigned long long* busy;  // [G]: shader cycles a workgroup spent on elements (not waiting), for `workgroups_busy`
    int32_t G, levels, qmax;
    uint32_t launch_id;  // (31 bits, unique in the process) travels in every message: what a ring still holds of an earlier launch - of
                         // this tree or of a tree whose memory it inherited - is never taken for a message, whatever a memset has or has not reached
    int32_t lvl_first[SYS_MAXLVL], lvl_count[SYS_MAXLVL];
};

constexpr u64 SYS_RES_NOSPLIT = 1, SYS_RES_SPLIT = 2;
__device__ __forceinline__ u64 sys_mail_word(uint32_t acked, uint32_t len, u64 res, uint32_t epoch = 0) {
    return (u64)acked | ((u64)len << 32) | (res << 48) | ((u64)(epoch & 0x3FFFu) << 50);  // (epoch: with a SPLIT result, the split's number)
}
// the epoch a 14-bit field stands for, given one this workgroup already knows (splits are far fewer than 2^13 apart)
__device__ __forceinline__ uint32_t sys_epoch_from(uint32_t known, u64 mailword) {
    const uint32_t d = ((uint32_t)(mailword >> 50) - known) & 0x3FFFu;
    return d < 0x2000u ? known + d : known;
}
__device__ __forceinline__ u64 sys_ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// "fresh" reads.  They were written as `fetch_add(p, 0)` - a read-modify-write, answered where the word lives - and that is
// NOT what ran: LLVM folds a relaxed `atomicrmw add p, 0` into a plain atomic load (its idempotent read-modify-write rule), so
// every build of this kernel polled with loads (the ISA of those builds has no returning 64-bit atomic at all).  Making the
// addend opaque (a zero loaded from a device global) gives the real read-modify-write - and breaks the kernel outright, in
// uncached, fine-grained and ordinary device memory alike (30 of 30 randomised runs, and the 1 M-row workloads): a returning
// atomic on a word another XCD stores to is not coherent with that store here.  profiles/r06/sys_fresh_reads_were_loads.txt.
// So these ARE loads, by name now, and what protects a wait is the invalidate between polls, not the kind of read.
__device__ __forceinline__ u64 sys_ld_fresh(u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }  // (global_load sc0 sc1: no better and no worse than sc1 in the randomised suite)
// (stores of the words workgroups talk through are atomic EXCHANGES, result unused: a waiter's read-modify-write read of a
// mailbox that raced with a plain store lost the store - the word went back to what the waiter had read - and the wait never
// ended: profiles/r06/sys_lost_store.txt.  Read-modify-writes are serialised against each other where the word lives.)
__device__ __forceinline__ void sys_st(u64* p, u64 v) { (void)__hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t sys_ld32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sys_st32(uint32_t* p, uint32_t v) { (void)__hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sys_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
__device__ __forceinline__ void sys_release() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the compiler may drop the wait behind buffer_wbl2: MI355X_MICROARCH.md)
}
// the hand-over of a quiesced chain (tree data written with plain stores by one workgroup, read with plain loads by another,
// possibly on another XCD): the strongest fences there are - system scope (buffer_wbl2 sc0 sc1 / buffer_inv sc0 sc1)
__device__ __forceinline__ void sys_acquire_chain() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, ""); }
__device__ __forceinline__ void sys_release_chain() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// A barrier behind which every wave's global STORES have been performed.  `__syncthreads()` on gfx950 is
// `s_waitcnt lgkmcnt(0); s_barrier`: it does not wait for stores (vmcnt), so a load another wave issues right behind it can
// reach L2 before the store it is meant to see (tools/probe/own_store_visibility.cpp shows the orderly case; the randomised
// suite at bf 254 - a node refilled, a leaf re-read one step after it was written - showed the other: hand-over counters
// that lost increments, stale centroid rows).  Every step of this kernel starts behind one.
__device__ __forceinline__ void sys_sync_mem() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}
__device__ __forceinline__ uint32_t sys_ld32_fresh(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ uint32_t sys_hash(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

// words of the kernel's own LDS block (behind the complete engine's layout): fixed words, then per mirrored node and row
// what the owner needs of the row besides the centroid (which the engine's mirror holds): the tracking row's cluster-feature
// slot and n_samples, the elements handed to the child, and the child's mailbox as last read
constexpr int SYS_MAXMIR = 8;
enum SysLds : int { SL_MSG_E = 0, SL_MSG_NODE, SL_MSG_ALONE, SL_MSG_EPOCH, SL_GOT, SL_TMP0, SL_TMP1, SL_TMP2, SL_VICTIM, SL_NSPLIT,
                    SL_HEAD = 16, SL_TAIL = SL_HEAD + SYS_MAXPROD, SL_MTAG = SL_TAIL + SYS_MAXPROD, SL_MLEN = SL_MTAG + SYS_MAXMIR,
                    SL_OWNACK = SL_MLEN + SYS_MAXMIR, SL_SPL = SL_OWNACK + SYS_MAXMIR /* split log: 4 words per split node */,
                    SL_FIXED = SL_SPL + 4 * SYS_MAXLVL };
enum SysRow : int { RS_SLOT = 0, RS_N, RS_SENT, RS_MACK, RS_MLEN, RS_WORDS = 8 };  // one 32-byte record per row: two LDS reads
template <class KCt> constexpr uint32_t sys_lds_bytes() { return (uint32_t)(SL_FIXED + RS_WORDS * KCt::nm * (int)KCt::rows) * 4u; }
static_assert(SL_FIXED % 4 == 0, "row records are read 16 bytes at a time");

// the kernel's own context type: the complete engine's fixed-shape context with as many LDS mirrors as the kernel wants
// (the engine sizes its own by the levels of ONE root-to-leaf path; an owner holds the nodes it owns)
template <int BF, int NM>
struct KSFix : KCBase {
    static constexpr bool dynamic_shape = false;
    static constexpr int F = 2048, nb = 256, RB = 256, RBc = 16, RBS = 272;
    static constexpr uint32_t rows = BF + 1, bf = BF, nblk = node_blocks(BF + 1);
    static constexpr int nm = NM;
    static constexpr Smem o = smem_layout(BF, 256, NM);
    static constexpr int buf = 0;          // packed fingerprints only
    static constexpr int crit_fixed = -1;  // the merge criterion is read at run time
    static_assert(NM <= SYS_MAXMIR, "mirror tags");
};

template <class KCt>
struct SysCtx {
    TreeDev* T;
    SysDev S;
    LA uint32_t* sl;
    uint32_t* gctr;
    int wg, level, me;       // this workgroup, the tree level it owns nodes of, its index inside the level
    int nprod, next_first, next_count;  // workgroups of the level above / first workgroup and workgroups of the level below
    uint32_t st_cmp, st_rows;           // statistics of the internal steps (compares, rows compared), folded in at the end
    uint32_t my_epoch;       // newest split this workgroup has acquired
    int red_slot, cmp_par;
    u64 t_busy;
    u64 ph[12];  // (phase-timer instance; [8] mailbox re-reads, [9] their spins, [10] ALONE hand-overs, [11] cycles waiting for them) cycles: lookup, compare (hit), fill + compare (miss), guard, send, commit, rest; [7] misses
    u64 tmark;
};
// phase timers of the internal step: only in the PROF instance of the kernel
#define PH(i) do { if constexpr (PROF) { const u64 _n = __builtin_amdgcn_s_memtime(); c.ph[i] += _n - c.tmark; c.tmark = _n; } } while (0)

// raise the abort flag (the line that gave up travels in it) - every wait looks at it
template <class KCt>
__device__ __forceinline__ void sys_abort(const SysCtx<KCt>& c, uint32_t line) {
    if (threadIdx.x == 0) {
        uint32_t expect = 0;
        __hip_atomic_compare_exchange_strong(c.S.ctl + SC_ABORT, &expect, line, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
template <class KCt>
__device__ __forceinline__ bool sys_aborted(const SysCtx<KCt>& c) {
    if (uni(sys_ld32(c.S.ctl + SC_ABORT)) == 0) return false;
    return uni(sys_ld32_fresh(c.S.ctl + SC_ABORT)) != 0;  // (a non-zero word is believed only when a read that cannot be stale says so too)
}

// element e of the call: packed row into LDS (o.x), popcount
template <class KCt>
__device__ __forceinline__ void sys_load_elem(const KCt& k, const SysCtx<KCt>& c, const uint8_t* rows, long long stride, uint32_t e, Elem& el) {
    const int tid = threadIdx.x;
    LA u32x4_t* sx = lds<u32x4_t>(k.L, k.o.x);
    if (tid < k.RBc) sx[tid] = ldg<u32x4_t>(rows + (size_t)e * (size_t)stride + (size_t)tid * 16);
    __syncthreads();
    el.idx = (long long)e;
    el.nS = 1;
    el.pcx = uni(lds_vec_popcount(k, k.o.x));
    el.s1S = el.pcx;
    el.s2S = el.pcx;
}

// one message to workgroup `cons` of the next level (thread 0; ring = (consumer, my index in my level))
template <class KCt>
__device__ __forceinline__ void sys_send(const SysCtx<KCt>& c, int cons_idx, uint32_t e, uint32_t node, bool alone) {
    if (threadIdx.x == 0) {
        const uint32_t cw = (uint32_t)(c.next_first + cons_idx);
        const uint32_t t = c.sl[SL_TAIL + cons_idx];
        u64* slot = c.S.rings + ((size_t)((cw * (uint32_t)SYS_MAXPROD + (uint32_t)c.me) * SYS_R + (t & (SYS_R - 1u)))) * 2;
        const u64 gen = (u64)(((t / SYS_R) + 1u) & 1u);
        sys_st(slot, (gen << 63) | ((u64)(alone ? 1u : 0u) << 62) | ((u64)node << 31) | (u64)e);
        sys_st(slot + 1, (gen << 63) | ((u64)(c.S.launch_id & 0x7FFFFFFFu) << 32) | (u64)c.my_epoch);
        c.sl[SL_TAIL + cons_idx] = t + 1;
    }
}
template <class KCt>
__device__ __forceinline__ int sys_owner_idx(const SysCtx<KCt>& c, uint32_t node) {
    // nodes are dealt to the owners of their level in the order their blocks were allocated (full-capacity nodes are KCt::nblk
    // blocks apart): consecutive nodes never share an owner - a hash put two hot 255-row nodes on one workgroup with one mirror
    return (int)((node / KCt::nblk) & ((uint32_t)c.next_count - 1u));  // (a power of two: sys_plan)
}

// Wait for the next message of this workgroup's rings (wave 0 polls every producer of the level above with one wave-wide
// load); false: the kernel is finishing or aborting.  The message lands in sl[SL_MSG_*].
template <class KCt>
__device__ __forceinline__ bool sys_poll(SysCtx<KCt>& c) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nprod = c.nprod;
    sys_state(c, 4, 0, 0, 0);
    if (tid < 64) {
        const uint32_t h = c.sl[SL_HEAD + (lane < nprod ? lane : 0)];
        const u64* slot = c.S.rings + ((size_t)(((uint32_t)c.wg * (uint32_t)SYS_MAXPROD + (uint32_t)(lane < nprod ? lane : 0)) * SYS_R + (h & (SYS_R - 1u)))) * 2;
        const u64 want_hi = ((u64)(((h / SYS_R) + 1u) & 1u) << 31) | (u64)(c.S.launch_id & 0x7FFFFFFFu);  // generation bit and launch id of half B's upper word
        const u64 gen = want_hi >> 31;
        uint32_t got = 0, empty = 0;
        while (true) {
            u64 a = 0, b = 0;
            bool ready = false;
            if (lane < nprod) {
                if ((empty & 7u) == 7u) {  // (every eighth look in a row that found nothing: reads that cannot be stale)
                    a = sys_ld_fresh((u64*)slot);
                    b = sys_ld_fresh((u64*)slot + 1);
                } else {
                    a = sys_ld(slot);
                    b = sys_ld(slot + 1);
                }
                ready = (a >> 63) == gen && (b >> 32) == want_hi;
            }
            const u64 m = __ballot(ready);
            if (m != 0ull) {
                const int p = __ffsll((long long)m) - 1;
                const u64 am = ((u64)rdlane((uint32_t)(a >> 32), p) << 32) | rdlane((uint32_t)a, p);
                const uint32_t ep = rdlane((uint32_t)b, p);
                if (lane == p) c.sl[SL_HEAD + p] = h + 1;
                if (lane == 0) {
                    c.sl[SL_MSG_E] = (uint32_t)(am & 0x7FFFFFFFull);
                    c.sl[SL_MSG_NODE] = (uint32_t)((am >> 31) & 0x3FFFFFFFull);
                    c.sl[SL_MSG_ALONE] = (uint32_t)((am >> 62) & 1ull);
                    c.sl[SL_MSG_EPOCH] = ep;
                }
                got = 1;
                break;
            }
            // nothing: finished / aborted?  Then look again - every fourth time behind an invalidate: a relaxed poll can stay
            // stale (tools/probe/oneway_stream.cpp), but an agent-scope acquire costs ~4 k cycles, which is what an element that
            // waits for this workgroup would pay on every hop
            // (SC_FINISH carries the launch id and a non-zero word is read again with a read that cannot be stale before it is
            // believed: the control words sit where the previous launch's did, and a workgroup that leaves on an old FINISH is a
            // consumer that never takes what its producers go on sending)
            uint32_t fin = 0;
            if (lane == 0) {
                const bool fresh = (empty & 7u) == 7u;
                uint32_t f = fresh ? sys_ld32_fresh(c.S.ctl + SC_FINISH) : sys_ld32(c.S.ctl + SC_FINISH);
                uint32_t ab = fresh ? sys_ld32_fresh(c.S.ctl + SC_ABORT) : sys_ld32(c.S.ctl + SC_ABORT);
                if (!fresh && (f != 0 || ab != 0)) {
                    const uint32_t f2 = sys_ld32_fresh(c.S.ctl + SC_FINISH), ab2 = sys_ld32_fresh(c.S.ctl + SC_ABORT);
                    if (f2 != f || ab2 != ab) atomicAdd(c.S.ctl + SC_STALE_CTL, 1u);
                    f = f2;
                    ab = ab2;
                }
                if (f != 0 && f != (0x80000000u | c.S.launch_id)) { atomicAdd(c.S.ctl + SC_STALE_CTL, 0x10000u); f = 0; }
                fin = f | ab;
            }
            if (rdlane(fin, 0) != 0) break;
            if ((++empty & (SYS_INV_EVERY - 1u)) == 0) sys_acquire();
            else __builtin_amdgcn_s_sleep(2);
        }
        if (lane == 0) c.sl[SL_GOT] = got;
    }
    sys_sync_mem();  // (what the previous step stored is in memory before this step reads anything)
    const bool ok = uni(c.sl[SL_GOT]) != 0;
    return ok;
}

// where a workgroup is waiting (read by the host when a wait gave up): kind (1 guard, 2 ALONE, 3 drain, 4 poll), node, child, want
template <class KCt>
__device__ __forceinline__ void sys_state(const SysCtx<KCt>& c, uint32_t kind, uint32_t node, uint32_t child, uint32_t want) {
    if (threadIdx.x == 0) {
        unsigned long long* st = c.S.busy + (size_t)c.S.G * 13 + (size_t)c.wg * 2;
        __hip_atomic_store(st, ((unsigned long long)kind << 32) | node, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(st + 1, ((unsigned long long)child << 32) | want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// spin until the child's mailbox shows `want` elements dealt with; returns the mailbox word (0 with the abort flag raised)
template <class KCt>
__device__ __forceinline__ u64 sys_wait_acked(const SysCtx<KCt>& c, uint32_t child, uint32_t want, uint32_t line) {
    const u64 t0 = __builtin_amdgcn_s_memtime();
    uint32_t spins = 0;
    while (true) {
        const u64 m = uni64((spins & 3u) == 3u ? sys_ld_fresh(c.S.mail + child) : sys_ld(c.S.mail + child));
        if ((uint32_t)m == want) return m;
        if (sys_aborted(c)) return 0;
        if (__builtin_amdgcn_s_memtime() - t0 > SYS_SPIN_LIMIT) { c.sl[SL_TMP0] = line; return 0; }
        if ((++spins & (SYS_INV_EVERY - 1u)) == 0) sys_acquire();
        else __builtin_amdgcn_s_sleep(2);
    }
}

// what an inconsistency looked like, for whoever reads the error (SysCtl words 8..15; first writer wins through the abort flag)
template <class KCt>
__device__ __forceinline__ void sys_dbg(const SysCtx<KCt>& c, uint32_t N, uint32_t C, uint32_t s, uint32_t mack, uint32_t info, uint32_t e) {
    if (threadIdx.x == 0 && sys_ld32(c.S.ctl + SC_ABORT) == 0) {
        c.S.ctl[8] = N; c.S.ctl[9] = C; c.S.ctl[10] = s; c.S.ctl[11] = mack;
        c.S.ctl[12] = ldg<uint32_t>(c.S.sent + C);
        c.S.ctl[13] = (uint32_t)sys_ld_fresh(c.S.mail + C);
        c.S.ctl[14] = info;
        c.S.ctl[15] = e;
    }
}

// `CF += x`, new majority centroid, popcount, n on tracking row (N, j) - bitbirch.py:352-357 - in HBM and in LDS mirror `ms`.
// `v` holds the row's cluster features for this thread's eight features, requested by the caller as soon as the row was
// chosen (the one memory round trip of a step that cannot be taken off its chain).
template <class KCt>
__device__ __forceinline__ void sys_commit(const KCt& k, SysCtx<KCt>& c, const Elem& el, uint32_t N, uint32_t j, uint32_t slotw, uint32_t n_old, int ms,
                                           uint32_t (&v)[8]) {
    const int tid = threadIdx.x;
    const size_t pm = (size_t)N * NG + j;
    const u64 n_new = (u64)n_old + el.nS;
    uint32_t cc[1] = {0};
    {
        const int b = tid;  // (2048-bit rows: one byte group per thread)
        uint32_t x8[8];
        elem_cols(k, el, b, x8);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] += x8[q];
        cf_store8(k, slotw, b, v);
        const uint32_t byte = centroid_byte(v, n_new);
        stg<uint8_t>(k.cent + pm * (size_t)k.RB + b, (uint8_t)byte);
        *(LA uint8_t*)(k.L + k.o.rc_cent + ((uint32_t)ms * k.rows + j) * k.RBS + b) = (uint8_t)byte;
        cc[0] = __popc(byte);
    }
    {
        // the new centroid's popcount: four wave sums through LDS, one barrier
        LA uint32_t* b32 = lds<uint32_t>(k.L, k.o.red32) + c.red_slot * TW * NRED;
        c.red_slot ^= 1;
        const uint32_t w = wsum32((uint32_t)cc[0]);
        if ((tid & 63) == 0) b32[(tid >> 6) * NRED] = w;
        __syncthreads();
        cc[0] = uni(b32[0] + b32[NRED] + b32[2 * NRED] + b32[3 * NRED]);
    }
    if (n_new > 0xFFFFFFFFull) sys_abort(c, __LINE__);
    if (tid == 0) {
        stg<uint32_t>((uint8_t*)(k.rm + pm) + 4, (uint32_t)n_new);
        stg<uint32_t>(k.card + pm, (uint32_t)cc[0]);
        lds<uint32_t>(k.L, k.o.rc_card)[(uint32_t)ms * k.rows + j] = (uint32_t)cc[0];
        c.sl[SL_FIXED + ((uint32_t)ms * k.rows + j) * RS_WORDS + RS_N] = (uint32_t)n_new;
    }
}

// Element e (its row in o.x) at internal node N: compare, guard, commit, hand over (the header comment).  `alone_in`: e
// reached N ALONE, i.e. N's parent has not committed and waits for N's mailbox.  Returns false when the kernel must stop
// admitting (the root was split under this very element, or an abort).
//
// The node sits in one of the owner's LDS mirrors (the engine's layout: centroids, popcounts, child ids) together with what
// else a step needs of a row - SysRow - so that a step on a resident node has ONE dependent memory round trip: the chosen
// tracking row's cluster features.  The child's mailbox is used as last read: every element the child has dealt with since
// is still counted as pending, and an element adds at most one row, so len_cached + pending_estimated bounds the truth from
// above - the word is read again only when that bound says "careful".
template <bool PROF, class KCt>
__device__ __forceinline__ bool sys_internal_step(const KCt& k, SysCtx<KCt>& c, const Elem& el, uint32_t e, uint32_t N, bool alone_in) {
    const int tid = threadIdx.x;
    LA uint32_t* sl = c.sl;
    if constexpr (PROF) c.tmark = __builtin_amdgcn_s_memtime();
    int ms = -1;
    {
        // (all tags with one LDS read: lane q looks at mirror q)
        static_assert(SYS_MAXMIR == 8, "tag lookup");
        const uint32_t q = (uint32_t)tid & 7u;
        const bool hit = q < (uint32_t)k.nm && sl[SL_MTAG + q] == N;
        const u64 mm = __ballot(hit) & 0xFFull;
        if (mm != 0ull) ms = __ffsll((long long)mm) - 1;
    }
    PH(0);
    uint32_t len = 0, j;
    bool anyc = true;
    const bool was_miss = ms < 0;
    if (ms < 0) {
        // bring the node in: rows, popcounts, child ids (node_best's fill), then the rows' records and the children's counters
        ms = (int)(uni(sl[SL_VICTIM]) % (uint32_t)k.nm);
        // (a fill is the one place where an owner takes a node's state from memory: behind an invalidate, whoever wrote it last -
        // this workgroup, a split's executor, the owner of the node it was split from)
        sys_sync_mem();
        sys_acquire_chain();
        uint32_t leafw = 0;
        const Cand best = node_best<false, false>(k, c.cmp_par, N, -1, k.o.x, el.pcx, false, false, true, &len, &leafw, (uint32_t)ms, true, &anyc);
        len = uni(len);
        if (hw_cap(uni(leafw)) < k.rows || (uni(leafw) & HW_LEAF) || len == 0) { sys_abort(c, __LINE__); return false; }  // (sealed / not internal: the host keeps such trees away)
        j = best.r;
        __syncthreads();  // (rc_link of every row is in LDS)
        for (uint32_t r = tid; r < len; r += TB) {
            const uint32_t ch = lds<uint32_t>(k.L, k.o.rc_link)[(uint32_t)ms * k.rows + r];
            const uint8_t* rmp = (const uint8_t*)(k.rm + (size_t)N * NG + r);
            const uint32_t rn = ldg<uint32_t>(rmp + 4), rslot = ldg<uint32_t>(rmp + 8);
            // (read-modify-write reads: `sent` and the mailbox are written with atomic exchanges, which are performed where these
            // reads are answered; a plain load may be served from a line this compute unit's L2 still holds from before the write -
            // this workgroup's own write included - and a `sent` that is too small makes the guard count too few elements below)
            const uint32_t sn = ldg<uint32_t>(c.S.sent + ch);
            const u64 m = sys_ld_fresh(c.S.mail + ch);
            sl[SL_FIXED + ((uint32_t)ms * k.rows + r) * RS_WORDS + RS_SLOT] = rslot;
            sl[SL_FIXED + ((uint32_t)ms * k.rows + r) * RS_WORDS + RS_N] = rn;
            sl[SL_FIXED + ((uint32_t)ms * k.rows + r) * RS_WORDS + RS_SENT] = sn;
            sl[SL_FIXED + ((uint32_t)ms * k.rows + r) * RS_WORDS + RS_MACK] = (uint32_t)m;
            sl[SL_FIXED + ((uint32_t)ms * k.rows + r) * RS_WORDS + RS_MLEN] = (uint32_t)(m >> 32) & 0xFFFFu;
        }
        if (tid == 0) {
            sl[SL_MTAG + ms] = N;
            sl[SL_MLEN + ms] = len;
            sl[SL_VICTIM] = sl[SL_VICTIM] + 1;
            sl[SL_OWNACK + ms] = c.level > 0 ? ldg<uint32_t>(c.S.acks + N) : 0u;  // (this node's own count, from its owner's own table)
        }
        __syncthreads();
        if constexpr (PROF) c.ph[7] += 1;
        PH(2);
    } else {
        len = uni(sl[SL_MLEN + ms]);
        const Cand best = node_best_mirror<false>(k, c.cmp_par, len, k.o.x, el.pcx, false, false, (uint32_t)ms, &anyc);
        j = best.r;
        PH(1);
    }
    const u32x4_t rr = *(LA u32x4_t*)(sl + SL_FIXED + ((uint32_t)ms * k.rows + j) * RS_WORDS);  // {slot, n, sent, acked}
    const uint32_t rlen = sl[SL_FIXED + ((uint32_t)ms * k.rows + j) * RS_WORDS + RS_MLEN];
    const uint32_t rC = lds<uint32_t>(k.L, k.o.rc_link)[(uint32_t)ms * k.rows + j];
    const uint32_t rack = sl[SL_OWNACK + ms];
    const uint32_t C = uni(rC), slotw = uni(rr.x), n_old = uni(rr.y), s = uni(rr.z);
    uint32_t mack = uni(rr.w), mlen = uni(rlen);
    const uint32_t my_acked = uni(rack);
    // invariants (cheap, always on): the child cannot have dealt with more than it was handed; elements reach a node in order
    if ((int32_t)(s - mack) < 0) {
        sys_dbg(c, N, C, s, mack, (uint32_t)c.level | ((uint32_t)was_miss << 8) | ((uint32_t)j << 16), e);
        sys_abort(c, __LINE__);
        return false;
    }
    {
        const uint32_t le = uni(ldg<uint32_t>(c.S.laste + N));
        if (le != 0 && e + 1 <= le) { sys_abort(c, __LINE__); return false; }
        if (tid == 0) stg<uint32_t>(c.S.laste + N, e + 1);
    }
    // the chosen row's cluster features: requested now, consumed by the commit
    uint32_t v[8];
    cf32_load8(k, slotw, tid, v);
    c.st_cmp += 1;
    c.st_rows += len;
    // guard: can C take one more row whatever the elements in flight below it do?
    bool alone = false;
    if (mlen + (s - mack) + 1 > k.bf) {
        const u64 t0 = __builtin_amdgcn_s_memtime();
        if constexpr (PROF) c.ph[8] += 1;
        sys_state(c, 1, N, C, s);
        uint32_t gspins = 0;
        while (true) {
            if constexpr (PROF) c.ph[9] += 1;
            const u64 m = uni64((gspins++ & 1u) ? sys_ld_fresh(c.S.mail + C) : sys_ld(c.S.mail + C));
            mack = (uint32_t)m;
            mlen = (uint32_t)(m >> 32) & 0xFFFFu;
            if ((int32_t)(s - mack) < 0) { sys_abort(c, __LINE__); return false; }
            if (mlen + (s - mack) + 1 <= k.bf) break;
            if (s == mack) { alone = true; break; }
            if (sys_aborted(c)) return false;
            if (__builtin_amdgcn_s_memtime() - t0 > SYS_SPIN_LIMIT) {
                sys_dbg(c, N, C, s, mack, (uint32_t)c.level | ((uint32_t)was_miss << 8) | ((uint32_t)j << 16) | 0x80u, e);
                sys_abort(c, __LINE__);
                return false;
            }
            sys_acquire();
        }
    }
    const int cons = sys_owner_idx(c, C);
    bool keep_going = true;
    // (the row's record in LDS is rewritten only behind a barrier that every wave passes AFTER it has read the record - the
    // commit's, or the one before the release below: the waves of a workgroup are not in lock step, and a wave that read
    // `sent` after thread 0 had bumped it would take a different turn at the guard)
    if (tid == 0) stg<uint32_t>(c.S.sent + C, s + 1);  // (kept in HBM too: the child may change parents - and owners of its parent - in a split)
    PH(3);
    if (!alone) {
        sys_send(c, cons, e, C, false);
        PH(4);
        sys_commit(k, c, el, N, j, slotw, n_old, ms, v);
        if (tid == 0) {
            LA uint32_t* rrow = sl + SL_FIXED + ((uint32_t)ms * k.rows + j) * RS_WORDS;
            rrow[RS_SENT] = s + 1;
            rrow[RS_MACK] = mack;
            rrow[RS_MLEN] = mlen;
            if (c.level > 0) {
                sys_st(c.S.mail + N, sys_mail_word(my_acked + 1, len, alone_in ? SYS_RES_NOSPLIT : 0));
                stg<uint32_t>(c.S.acks + N, my_acked + 1);
                sl[SL_OWNACK + ms] = my_acked + 1;
            }
        }
        PH(5);
    } else {
        // C is full and nothing is in flight below it: e goes down ALONE, this row is left as it is until e's fate is known
        if (len >= k.bf) {
            // This node is full as well: if C splits, so does this node, and the rows that move to the new node get a new
            // producer - the new node's owner.  A ring is first-in first-out per PRODUCER: whatever this workgroup has handed to
            // any of its children must have been taken out of their rings before a later element can reach them through another
            // workgroup.  (Found by the randomised suite at bf 254: an element overtook an earlier one of the same leaf.)
            const u64 t0 = __builtin_amdgcn_s_memtime();
            sys_state(c, 3, N, C, s);
            for (uint32_t r = tid; r < len; r += TB) {
                const uint32_t ch = lds<uint32_t>(k.L, k.o.rc_link)[(uint32_t)ms * k.rows + r];
                const uint32_t sn = sl[SL_FIXED + ((uint32_t)ms * k.rows + r) * RS_WORDS + RS_SENT];
                uint32_t spins = 0;
                while (r != j && (uint32_t)((spins & 1u) ? sys_ld_fresh(c.S.mail + ch) : sys_ld(c.S.mail + ch)) != sn) {  // (row j: nothing pending, or e would not go ALONE)
                    if (sys_ld32(c.S.ctl + SC_ABORT) != 0) break;
                    if (__builtin_amdgcn_s_memtime() - t0 > SYS_SPIN_LIMIT) { sys_abort(c, __LINE__); break; }
                    if ((++spins & (SYS_INV_EVERY - 1u)) == 0) sys_acquire();
                    else __builtin_amdgcn_s_sleep(2);
                }
            }
            __syncthreads();
            if (sys_aborted(c)) return false;
        }
        if (tid == 0) stg<u64>(c.S.up + C, ((u64)N << 32) | j);
        sys_sync_mem();
        if (tid == 0) sl[SL_FIXED + ((uint32_t)ms * k.rows + j) * RS_WORDS + RS_SENT] = s + 1;
        sys_release_chain();  // (whoever splits below reads this node's rows, records and tracking cluster features)
        sys_send(c, cons, e, C, true);
        sys_state(c, 2, N, C, s + 1);
        const u64 tw0 = PROF ? __builtin_amdgcn_s_memtime() : 0;
        const u64 m2 = sys_wait_acked(c, C, s + 1, __LINE__);
        if constexpr (PROF) { c.ph[10] += 1; c.ph[11] += __builtin_amdgcn_s_memtime() - tw0; }
        if (m2 == 0) {
            sys_dbg(c, N, C, s + 1, mack, (uint32_t)c.level | ((uint32_t)was_miss << 8) | ((uint32_t)j << 16) | 0x40u, e);
            sys_abort(c, __LINE__);
            return false;
        }
        const u64 res = (m2 >> 48) & 3ull;
        if (tid == 0) {
            sl[SL_FIXED + ((uint32_t)ms * k.rows + j) * RS_WORDS + RS_MACK] = (uint32_t)m2;
            sl[SL_FIXED + ((uint32_t)ms * k.rows + j) * RS_WORDS + RS_MLEN] = (uint32_t)(m2 >> 32) & 0xFFFFu;
        }
        if (res == SYS_RES_NOSPLIT) {
            sys_commit(k, c, el, N, j, slotw, n_old, ms, v);
            if (c.level > 0 && tid == 0) {
                sys_st(c.S.mail + N, sys_mail_word(my_acked + 1, len, alone_in ? SYS_RES_NOSPLIT : 0));
                stg<uint32_t>(c.S.acks + N, my_acked + 1);
                sl[SL_OWNACK + ms] = my_acked + 1;
            }
        } else if (res == SYS_RES_SPLIT) {
            // C was split: row j and a new row were written by the leaf's owner (update_split_subclusters, bitbirch.py:289-303),
            // and if this node was full it has been split as well (its mailbox written for it): reload
            sys_acquire_chain();
            c.my_epoch = sys_epoch_from(c.my_epoch, m2);  // (the split's number came with the word this workgroup waited for: not another - possibly stale - read)
            if (tid == 0) sl[SL_MTAG + ms] = NONE;
            __syncthreads();
            if (len >= k.bf) {
                if (c.level == 0) keep_going = false;  // the root itself: depth and root changed, the host relaunches
            } else if (c.level > 0 && tid == 0) {
                sys_st(c.S.mail + N, sys_mail_word(my_acked + 1, len + 1, alone_in ? SYS_RES_NOSPLIT : 0));
                stg<uint32_t>(c.S.acks + N, my_acked + 1);
            }
        } else {
            sys_abort(c, __LINE__);
            return false;
        }
    }
    // (no barrier here: whatever thread 0 has just written to LDS - the row's popcount and n, the counters - is read by the next
    // step behind the barrier that follows its element's arrival in o.x)
    PH(6);
    return keep_going;
}
#undef PH

// Element e (row in o.x) at leaf L: bitbirch.py:321-337 with the complete engine's arithmetic (tree_insert_body, D = 0), then
// - ALONE elements only - the split cascade.  Writes out_leaf[e], the leaf's mailbox, the completion counter.
template <class KCt>
__device__ __forceinline__ void sys_leaf_step(const KCt& k, SysCtx<KCt>& c, const Elem& el, uint32_t e, uint32_t L, bool alone, uint32_t* out_leaf) {
    const int tid = threadIdx.x;
    uint32_t* gctr = c.gctr;
    LA u64* stats = lds<u64>(k.L, k.o.stats);
    LA uint32_t* bc = lds<uint32_t>(k.L, k.o.bc);
    const uint32_t bf = k.bf;
    const int nb = k.nb;
    u64 mail_old = 0;  // (the leaf's own count, consumed at the end: the round trip hides under the step; an old value would make it count backwards)
    if (tid == 0) mail_old = ldg<uint32_t>(c.S.acks + L);
    {
        const uint32_t le = uni(ldg<uint32_t>(c.S.laste + L));
        if (le != 0 && e + 1 <= le) { sys_abort(c, __LINE__); return; }
        if (tid == 0) stg<uint32_t>(c.S.laste + L, e + 1);
    }
    uint32_t len = 0, leafw = 0;
    bool anyc = true;
    const Cand best = node_best<false, false>(k, c.cmp_par, L, -1, k.o.x, el.pcx, false, false, true, &len, &leafw, 0u, false, &anyc);
    len = uni(len);
    leafw = uni(leafw);
    if (hw_cap(leafw) < k.rows || !(leafw & HW_LEAF) || len == 0) { sys_abort(c, __LINE__); return; }
    const uint32_t jl = best.r, leaflen = len;
    const uint32_t slotT = uni(lds<uint32_t>(k.L, k.o.link)[c.cmp_par * k.rows + jl]);
    const uint8_t* rmp = (const uint8_t*)(k.rm + (size_t)L * NG + jl);
    const u32x4_t rm0 = ldg<u32x4_t>(rmp), rm1 = ldg<u32x4_t>(rmp + 16);
    if (tid == 0) {
        stats[0]++;
        stats[1] += len;
    }
    const int b0 = tid;
    const bool act = b0 < nb;  // (rows of <= 2048 bits: one byte group per thread)
    u32x4_t rawL[2] = {(u32x4_t)(0), (u32x4_t)(0)};
    const uint8_t* const crowT = k.cent + ((size_t)L * NG + jl) * (size_t)k.RB;
    uint32_t cbyteT = 0;
    if (act) {
        cf_load_raw(k, slotT, b0, rawL);
        cbyteT = ldg<uint8_t>(crowT + b0);
    }
    const uint32_t Tsub = uni(rm0.x);
    const u64 nT = uni(rm0.y);
    const u64 s1T = ((u64)uni(rm1.y) << 32) | uni(rm1.x);
    const u64 s2T = ((u64)uni(rm1.w) << 32) | uni(rm1.z);
    const u64 new_n = nT + el.nS;
    if (new_n > 0xFFFFFFFFull) { sys_abort(c, __LINE__); return; }
    const uint32_t slotE = slot_effective(slotT, nT);
    if (nT == 1) { rawL[0] = (u32x4_t)(0); rawL[0].x = cbyteT; }
    u64 dot = 0;
    uint32_t pcs[1 + MAXFAST];
#pragma unroll
    for (int i = 0; i < 1 + MAXFAST; ++i) pcs[i] = 0;
    uint32_t xs[8], vL[8], byteL = 0;
    const bool wide_dot = (slotT >> 30) == 2;
    if (act) {
        elem_cols(k, el, b0, xs);
        cf_unpack_raw(slotE >> 30, rawL, vL);
        if (wide_dot) {
#pragma unroll
            for (int q = 0; q < 8; ++q) dot += (u64)vL[q] * xs[q];
        } else {
            uint32_t d32 = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) d32 += vL[q] * xs[q];
            dot = d32;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) vL[q] += xs[q];
        byteL = centroid_byte_merged(vL, new_n);
        pcs[0] = __popc(byteL);
    }
    block_sum_fused(k, c.red_slot, wide_dot, dot, pcs, 1);
    const u64 s1n = s1T + el.s1S;
    const u64 s2n = s2T + 2ull * dot + el.s2S;
    const bool accept = merge_accept(k, el, c.red_slot, slotE, crowT, nT, s1T, s2T, new_n, s1n, s2n);
    const size_t leafm = (size_t)L * NG;
    uint32_t out_id, new_len = leaflen;
    bool overflow = false;
    uint32_t dN = 0, d32c = 0, dF = 0;  // (allocation happens through the tree's counters: SUB mode of alloc_n)
    if (accept) {
        const uint32_t old_tier = slotT >> 30;
        const uint32_t new_tier = tier_for(new_n) > old_tier ? tier_for(new_n) : old_tier;
        uint32_t slotN = slotT;
        if (new_tier != old_tier) {
            slotN = (new_tier << 30) | (new_tier == 1 ? alloc_n<true>(k, dN, gctr + C_N16, 1, 15) : alloc_n<true>(k, dN, gctr + C_N32, 1, 15));
        } else if (nT == 1) {
            slotN = alloc_n<true>(k, dN, gctr + C_N8, 1, 15);
        }
        uint8_t* crow = k.cent + (leafm + jl) * (size_t)k.RB;
        if (act) {
            cf_store8(k, slotN, b0, vL);
            stg<uint8_t>(crow + b0, (uint8_t)byteL);
        }
        if (tid == 0) {
            u32x4_t a, b;
            a.x = Tsub; a.y = (uint32_t)new_n; a.z = slotN; a.w = 0;
            b.x = (uint32_t)s1n; b.y = (uint32_t)(s1n >> 32); b.z = (uint32_t)s2n; b.w = (uint32_t)(s2n >> 32);
            stg<u32x4_t>((uint8_t*)(k.rm + leafm + jl), a);
            stg<u32x4_t>((uint8_t*)(k.rm + leafm + jl) + 16, b);
            stg<uint32_t>(k.card + leafm + jl, pcs[0]);
            if (slotN != slotT) stg<uint32_t>(k.link + leafm + jl, slotN);
            stats[2]++;
        }
        out_id = Tsub;
    } else {
        // append_subcluster (bitbirch.py:284-287): a fingerprint's cluster features are its centroid row (SLOT_LAZY8)
        const uint32_t sid = alloc_n<true>(k, dN, gctr + C_IDS, 1, 14);
        if (tid == 0) {
            stg<uint32_t>(k.hdr + L, leaflen + 1);
            stats[3]++;
        }
        node_put_row(k, L, leaflen, k.o.x, el.pcx, SLOT_LAZY8, sid, el.nS, SLOT_LAZY8, el.s1S, el.s2S);
        out_id = sid;
        new_len = leaflen + 1;
        overflow = leaflen + 1 > bf;
    }
    if (tid == 0 && out_leaf) stg<uint32_t>(out_leaf + e, out_id);
    u64 res = alone ? SYS_RES_NOSPLIT : 0;
    if (overflow) {
        if (!alone) { sys_abort(c, __LINE__); return; }  // (the guard lets a leaf overflow under an ALONE element only)
        // ---- the split cascade (tree_insert_body's overflow loop on the quiesced chain) ----------------------------------
        sys_sync_mem();  // (the appended row is in memory)
        sys_acquire_chain();
        u64 sph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t nd = L, nsplit = 0;
        bool bad = false;
        while (true) {
            const u64 upw = uni64(ldg<u64>(c.S.up + nd));
            const uint32_t P = (uint32_t)(upw >> 32), jp = (uint32_t)upw;
            uint32_t trk = NONE, lenP = 0;
            if (P != NONE) {
                trk = uni(ldg<uint32_t>((const uint8_t*)(k.rm + (size_t)P * NG + jp) + 8));
                lenP = uni(ldg<uint32_t>(k.hdr + P));
            }
            split_node<true, false>(k, el, c.red_slot, c.cmp_par, nd, 0u, false, trk, dN, d32c, dF, gctr, sph);
            const uint32_t node1 = uni(bc[0]), cardA = uni(bc[3]), cardB = uni(bc[4]);
            const uint32_t nA = uni(bc[7]), nB = uni(bc[8]), n1 = uni(bc[5]), n2 = uni(bc[6]);
            const uint32_t slotA = (2u << 30) | uni(bc[9]), slotB = (2u << 30) | uni(bc[10]);
            if (uni(bc[11]) || nsplit >= (uint32_t)SYS_MAXLVL) { bad = true; break; }
            if (tid == 0) {
                c.sl[SL_SPL + 4 * nsplit + 0] = nd; c.sl[SL_SPL + 4 * nsplit + 1] = n2;
                c.sl[SL_SPL + 4 * nsplit + 2] = node1; c.sl[SL_SPL + 4 * nsplit + 3] = n1;
            }
            nsplit++;
            if (P == NONE) {
                // root split: a new root with the two tracking BitFeatures (bitbirch.py:778-782)
                const uint32_t nr = alloc_n<true>(k, dN, gctr + C_NODES, k.nblk, 14);
                node_put_row(k, nr, 0, k.o.cA, cardA, node1, NONE, nA, slotA, 0, 0);
                node_put_row(k, nr, 1, k.o.cB, cardB, nd, NONE, nB, slotB, 0, 0);
                if (tid == 0) {
                    u32x4_t h;
                    h.x = 2; h.y = hw_make(0u, k.rows); h.z = NONE; h.w = NONE;
                    stg<u32x4_t>(k.hdr + nr, h);
                    stats[5]++;
                    stg<uint32_t>(gctr + C_ROOT, nr);
                    atomicAdd(gctr + C_DEPTH, 1u);
                    sys_st32(c.S.ctl + SC_STOP, (uint32_t)STOP_SYS_RELAUNCH);
                }
                break;
            }
            node_put_row(k, P, jp, k.o.cA, cardA, node1, NONE, nA, slotA, 0, 0);
            node_put_row(k, P, lenP, k.o.cB, cardB, nd, NONE, nB, slotB, 0, 0);
            if (tid == 0) stg<uint32_t>(k.hdr + P, lenP + 1);
            sys_sync_mem();  // (the parent's two rows are in memory before its own split reads them)
            if (lenP + 1 > bf) { nd = P; continue; }
            break;
        }
        if (bad) { sys_abort(c, __LINE__); return; }
        __syncthreads();
        // the new nodes' mailboxes and counters, then everything out (release), then the split nodes' mailboxes - the words
        // their parents' owners are waiting on
        if (tid == 0) {
            for (uint32_t i = 0; i < nsplit; ++i) {
                const uint32_t node1 = c.sl[SL_SPL + 4 * i + 2], n1 = c.sl[SL_SPL + 4 * i + 3];
                sys_st(c.S.mail + node1, sys_mail_word(0, n1, 0));
                stg<uint32_t>(c.S.sent + node1, 0u);
                stg<uint32_t>(c.S.acks + node1, 0u);
                stg<uint32_t>(c.S.laste + node1, 0u);
                if (i >= 1) {  // a split internal node of the chain: its count goes up by the lone element, here, on its owner's behalf
                    const uint32_t x = c.sl[SL_SPL + 4 * i + 0];
                    const uint32_t ax = ldg<uint32_t>(c.S.acks + x) + 1u;
                    stg<uint32_t>(c.S.acks + x, ax);
                    c.sl[SL_SPL + 4 * i + 3] = ax;  // (n1 is not needed again)
                }
            }
        }
        sys_sync_mem();
        sys_release_chain();
        if (tid == 0) bc[12] = atomicAdd(c.S.ctl + SC_EPOCH, 1u) + 1u;
        __syncthreads();
        c.my_epoch = uni(bc[12]);
        // `my_epoch` = k means "every split up to k has been acquired by this workgroup": a message tagged <= k triggers no
        // invalidate.  This workgroup last acquired when its cascade STARTED; a cascade of another executor may have released
        // and taken a smaller number since (numbers are handed out at the end), and its results - a new leaf this workgroup
        // owns, rows moved between nodes - would be read from stale lines.  (Found late in round 6 from where the randomised
        // suite's different trees first differ: the element right behind another leaf's split.)
        sys_acquire_chain();
        if (tid == 0) {
            for (uint32_t i = 1; i < nsplit; ++i) {  // (internal nodes of the chain; the leaf's own word is written below)
                const uint32_t x = c.sl[SL_SPL + 4 * i + 0], n2 = c.sl[SL_SPL + 4 * i + 1];
                sys_st(c.S.mail + x, sys_mail_word(c.sl[SL_SPL + 4 * i + 3], n2, SYS_RES_SPLIT, c.my_epoch));
            }
        }
        new_len = uni(c.sl[SL_SPL + 1]);
        res = SYS_RES_SPLIT;
        __syncthreads();
    }
    if (tid == 0) {
        stg<uint32_t>(c.S.acks + L, (uint32_t)mail_old + 1);
        sys_st(c.S.mail + L, sys_mail_word((uint32_t)mail_old + 1, new_len, res, c.my_epoch));
        atomicAdd(c.S.ctl + SC_COMPLETED, 1u);
    }
    __syncthreads();
}

template <class KCt, bool PROF = false>
__global__ __launch_bounds__(TB) void k_tree_sys(TreeDev* T, SysDev S) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    KCt k;
    k.cent = T->node_cent; k.card = T->node_card; k.link = T->node_link; k.rm = T->node_rm; k.hdr = T->node_hdr;
    k.scratch = T->scratch_cent; k.cf8 = T->cf8; k.cf16 = T->cf16; k.cf32 = T->cf32;
    k.bufs = nullptr; k.width = 0;
    k.crit = (int)uni((uint32_t)T->crit); k.tol_len = (int)uni((uint32_t)T->tol_len); k.thr = T->thr; k.tolerance = T->tolerance; k.tol = T->tol_table;
    k.L = (LA unsigned char*)smem_raw;
    const int tid = threadIdx.x;
    SysCtx<KCt> c;
    c.T = T; c.S = S; c.sl = (LA uint32_t*)(k.L + k.o.total); c.gctr = T->ctr;
    constexpr int SL_WORDS = (int)(sys_lds_bytes<KCt>() / 4);
    c.wg = (int)blockIdx.x; c.level = 0; c.me = 0; c.my_epoch = 0; c.red_slot = 0; c.cmp_par = 0; c.t_busy = 0; c.tmark = 0;
    for (int i = 0; i < 12; ++i) c.ph[i] = 0;
    for (int l = 0; l < S.levels; ++l)
        if (c.wg >= S.lvl_first[l] && c.wg < S.lvl_first[l] + S.lvl_count[l]) { c.level = l; c.me = c.wg - S.lvl_first[l]; }
    c.level = (int)uni((uint32_t)c.level);
    c.me = (int)uni((uint32_t)c.me);
    c.nprod = 0; c.next_first = 0; c.next_count = 1; c.st_cmp = 0; c.st_rows = 0;
    for (int l = 0; l < S.levels; ++l) {
        if (l == c.level - 1) c.nprod = S.lvl_count[l];
        if (l == c.level + 1) { c.next_first = S.lvl_first[l]; c.next_count = S.lvl_count[l]; }
    }
    c.nprod = (int)uni((uint32_t)c.nprod); c.next_first = (int)uni((uint32_t)c.next_first); c.next_count = (int)uni((uint32_t)c.next_count);
    LA u64* stats = lds<u64>(k.L, k.o.stats);
    for (int i = tid; i < SL_WORDS; i += TB) c.sl[i] = (i >= SL_MTAG && i < SL_MTAG + SYS_MAXMIR) ? NONE : 0u;
    if (tid < 8) stats[tid] = 0ull;
    for (int ch = tid; ch < k.RBc; ch += TB) lds<u32x4_t>(k.L, k.o.x)[ch] = (u32x4_t)(0);
    __syncthreads();
    const uint8_t* rows = T->rows;
    const long long stride = T->row_stride;
    uint32_t* out_leaf = T->out_leaf;
    const bool leaf_level = c.level == S.levels - 1;
    Elem el;
    if (c.wg == 0) {
        // ---- level 0: admits the elements in order and owns the root -------------------------------------------------------
        const uint32_t n = (uint32_t)T->n_elems;
        const uint32_t root = uni(T->ctr[C_ROOT]), depth = uni(T->ctr[C_DEPTH]);
        const uint32_t cap_nodes = uni(T->cap_nodes), cap8 = uni(T->cap8), cap16 = uni(T->cap16), cap32 = uni(T->cap32);
        // what the elements in flight can take in the worst case (every one of them splits every level and a new root)
        const uint32_t q = (uint32_t)S.qmax + 64u;
        const uint32_t need_nodes = q * (depth + 2) * k.nblk, need32 = q * 2 * (depth + 2), need8 = q, need16 = q;
        int stop = STOP_DONE;
        uint32_t e = 0, completed = 0;
        u64 t_progress = __builtin_amdgcn_s_memtime();
        u32x4_t pf = (u32x4_t)(0);
        if (n > 0 && tid < k.RBc) pf = ldg<u32x4_t>(rows + (size_t)tid * 16);
        for (; e < n; ++e) {
            if ((e & 63u) == 0) {
                // (read-modify-write reads: they are answered where the owners' atomic adds are performed.  A relaxed load can return a
                // stale line - tools/probe/oneway_stream.cpp - and a stale-LOW counter admits elements the pools have no room for:
                // found by the randomised suite with pools that run out, 1 run in 40, a cluster-feature slot past the pool's end)
                __syncthreads();
                if (tid == 0) {
                    c.sl[SL_TMP0] = sys_ld32_fresh(T->ctr + C_NODES);
                    c.sl[SL_TMP1] = sys_ld32_fresh(T->ctr + C_N8);
                    c.sl[SL_TMP2] = sys_ld32_fresh(T->ctr + C_N16);
                    c.sl[SL_NSPLIT] = sys_ld32_fresh(T->ctr + C_N32);
                }
                __syncthreads();
                const uint32_t cN = uni(c.sl[SL_TMP0]), c8 = uni(c.sl[SL_TMP1]), c16 = uni(c.sl[SL_TMP2]), c32 = uni(c.sl[SL_NSPLIT]);
                if (cN + need_nodes > cap_nodes) { stop = STOP_NODES; break; }
                if (c8 + need8 > cap8) { stop = STOP_CF8; break; }
                if (c16 + need16 > cap16) { stop = STOP_CF16; break; }
                if (c32 + need32 > cap32) { stop = STOP_CF32; break; }
                const uint32_t sr = uni(sys_ld32_fresh(S.ctl + SC_STOP));
                if (sr != 0) { stop = (int)sr; break; }
                if (sys_aborted(c)) break;
            }
            // at most qmax elements in flight: no ring can overflow, and the reserve above covers them
            while (e - completed >= (uint32_t)S.qmax) {
                const uint32_t cnow = uni(sys_ld32_fresh(S.ctl + SC_COMPLETED));
                if (cnow != completed) { completed = cnow; t_progress = __builtin_amdgcn_s_memtime(); continue; }
                if (sys_aborted(c)) break;
                if (__builtin_amdgcn_s_memtime() - t_progress > SYS_SPIN_LIMIT) { sys_abort(c, __LINE__); break; }
                sys_acquire();
            }
            if (e - completed >= (uint32_t)S.qmax) break;  // (left the wait on an abort)
            const u64 tb = __builtin_amdgcn_s_memtime();
            {
                // (this row was requested while the previous element was dealt with; the next one is requested now)
                LA u32x4_t* sx = lds<u32x4_t>(k.L, k.o.x);
                if (tid < k.RBc) sx[tid] = pf;
                sys_sync_mem();  // (what the previous step stored is in memory before this step reads anything)
                if (e + 1 < n && tid < k.RBc) pf = ldg<u32x4_t>(rows + (size_t)(e + 1) * (size_t)stride + (size_t)tid * 16);
                el.idx = (long long)e;
                el.nS = 1;
                el.pcx = uni(lds_vec_popcount(k, k.o.x));
                el.s1S = el.pcx;
                el.s2S = el.pcx;
            }
            const bool go = sys_internal_step<PROF>(k, c, el, e, root, false);
            c.t_busy += __builtin_amdgcn_s_memtime() - tb;
            if (!go) { ++e; if (!sys_aborted(c)) stop = STOP_SYS_RELAUNCH; break; }
        }
        // drain: everything admitted has to arrive at its leaf
        t_progress = __builtin_amdgcn_s_memtime();
        while (!sys_aborted(c)) {
            const uint32_t cnow = uni(sys_ld32_fresh(S.ctl + SC_COMPLETED));
            if (cnow == e) break;
            if (cnow != completed) { completed = cnow; t_progress = __builtin_amdgcn_s_memtime(); }
            if (__builtin_amdgcn_s_memtime() - t_progress > SYS_SPIN_LIMIT) { sys_abort(c, __LINE__); break; }
            sys_acquire();
        }
        const uint32_t ab = uni(sys_ld32_fresh(S.ctl + SC_ABORT));
        if (tid == 0) {
            if (stop == STOP_DONE) {  // (a root split signalled while the last elements were on their way)
                const uint32_t sr = sys_ld32_fresh(S.ctl + SC_STOP);
                if (sr != 0 && e < n) stop = (int)sr;
            }
            T->processed = (long long)e;
            T->stop_reason = ab != 0 ? STOP_INTERNAL : stop;
            T->giveup_line = ab;
            sys_st32(S.ctl + SC_ADMITTED, e);
            sys_st32(S.ctl + SC_FINISH, 0x80000000u | S.launch_id);
        }
    } else if (!leaf_level) {
        while (sys_poll(c)) {
            const u64 tb = __builtin_amdgcn_s_memtime();
            const uint32_t e = uni(c.sl[SL_MSG_E]), N = uni(c.sl[SL_MSG_NODE]), ep = uni(c.sl[SL_MSG_EPOCH]);
            const bool alone = uni(c.sl[SL_MSG_ALONE]) != 0;
            __syncthreads();
            if ((int32_t)(ep - c.my_epoch) > 0) {  // a split this workgroup has not seen the results of: the node may be new to it
                sys_acquire_chain();
                c.my_epoch = ep;
            }
            sys_load_elem(k, c, rows, stride, e, el);
            sys_state(c, 5, N, e, alone ? 1u : 0u);
            (void)sys_internal_step<PROF>(k, c, el, e, N, alone);
            c.t_busy += __builtin_amdgcn_s_memtime() - tb;
            if (sys_aborted(c)) break;
        }
    } else {
        while (sys_poll(c)) {
            const u64 tb = __builtin_amdgcn_s_memtime();
            const uint32_t e = uni(c.sl[SL_MSG_E]), L = uni(c.sl[SL_MSG_NODE]), ep = uni(c.sl[SL_MSG_EPOCH]);
            const bool alone = uni(c.sl[SL_MSG_ALONE]) != 0;
            __syncthreads();
            if ((int32_t)(ep - c.my_epoch) > 0) {
                sys_acquire_chain();
                c.my_epoch = ep;
            }
            sys_load_elem(k, c, rows, stride, e, el);
            sys_state(c, 6, L, e, alone ? 1u : 0u);
            sys_leaf_step(k, c, el, e, L, alone, out_leaf);
            c.t_busy += __builtin_amdgcn_s_memtime() - tb;
            if (sys_aborted(c)) break;
        }
    }
    if (tid == 0) {
        stats[0] += c.st_cmp;
        stats[1] += c.st_rows;
    }
    __syncthreads();
    // statistics of this workgroup into the tree's (bbh_tree_stats: compares, rows compared, merges, appends, splits)
    if (tid < 6) atomicAdd((unsigned long long*)&T->stats[tid], (unsigned long long)stats[tid]);
    if (tid == 6 && leaf_level) atomicMax((unsigned long long*)&T->stats[6], (unsigned long long)S.levels);
    // (debugging aid: this workgroup's ring positions - messages taken per producer, messages sent per consumer)
    if (tid < 2 * SYS_MAXPROD) ((uint32_t*)(S.busy + (size_t)S.G * 15))[(size_t)c.wg * 2 * SYS_MAXPROD + tid] = c.sl[SL_HEAD + tid];
    if (tid == 0) {
        S.busy[c.wg] = c.t_busy;
        if constexpr (PROF)
            for (int i = 0; i < 12; ++i) S.busy[(size_t)S.G + (size_t)c.wg * 12 + i] = c.ph[i];
    }
}

// mailboxes and hand-over counters of every node, from the headers (one thread per block of the node pool)
__global__ __launch_bounds__(256) void k_sys_init(const NodeHdr* __restrict__ hdr, uint32_t used, u64* mail, uint32_t* sent, u64* up, uint32_t* laste, uint32_t* acks) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= used) return;
    const u32x4_t h = ldg<u32x4_t>(hdr + b);
    sys_st(mail + b, sys_mail_word(0, h.x & 0xFFFFu, 0));
    sent[b] = 0;
    laste[b] = 0;
    acks[b] = 0;
    up[b] = ((u64)NONE << 32);
}

// ---- BitFeature ids in the reference's order ---------------------------------------------------------------------------
// The sequential engines hand out BitFeature ids in insertion order (the id of an appended BitFeature is the number of
// BitFeatures created before it); here whichever leaf owner appends first takes the next id.  After a launch the ids it
// handed out are renumbered by the position of their CREATING element - the smallest element that ended in the BitFeature:
// an element can only merge into what earlier elements created - so that `out_leaf` and the rows' records are exactly what
// the sequential engines (and the oracle) produce.
__global__ __launch_bounds__(256) void k_sys_creator(const uint32_t* __restrict__ out_leaf, uint32_t n, uint32_t base, uint32_t* creator) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const uint32_t id = out_leaf[e];
    if (id >= base && id != NONE) atomicMin(creator + (id - base), e);
}
__global__ __launch_bounds__(256) void k_sys_flag(const uint32_t* __restrict__ out_leaf, uint32_t n, uint32_t base, const uint32_t* __restrict__ creator,
                                                  uint32_t* __restrict__ flag) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const uint32_t id = out_leaf[e];
    flag[e] = (id >= base && id != NONE && creator[id - base] == e) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_sys_map(const uint32_t* __restrict__ creator, const uint32_t* __restrict__ rank, uint32_t nnew, uint32_t base,
                                                 uint32_t* __restrict__ map) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnew) return;
    const uint32_t cr = creator[i];
    map[i] = cr == NONE ? base + i : base + rank[cr];  // (an id nobody ended in cannot exist: kept as it is)
}
__global__ __launch_bounds__(256) void k_sys_apply_out(uint32_t* __restrict__ out_leaf, uint32_t n, uint32_t base, uint32_t nnew, const uint32_t* __restrict__ map) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const uint32_t id = out_leaf[e];
    if (id >= base && id - base < nnew) out_leaf[e] = map[id - base];
}
// one wave per block of the node pool: the rows of every leaf that starts there
__global__ __launch_bounds__(256) void k_sys_apply_rows(const NodeHdr* __restrict__ hdr, RowMeta* __restrict__ rm, uint32_t used, uint32_t base, uint32_t nnew,
                                                        const uint32_t* __restrict__ map) {
    const uint32_t b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (b >= used) return;
    const u32x4_t h = ldg<u32x4_t>(hdr + b);
    if (hw_cap(h.y) == 0 || !(h.y & HW_LEAF)) return;
    for (uint32_t r = lane; r < h.x; r += 64) {
        uint32_t* sub = (uint32_t*)(rm + (size_t)b * NG + r);
        const uint32_t id = *sub;
        if (id >= base && id - base < nnew) *sub = map[id - base];
    }
}

using KS50 = KSFix<50, 8>;    // eight mirrored nodes per owner (136 KB + 9 KB of per-row words)
using KS254 = KSFix<254, 1>;  // one 255-row node per owner (117 KB + 5 KB)

#endif  // __HIPCC__
