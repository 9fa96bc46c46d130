// Everything the host does for the level-systolic kernel (bb_tree_sys.inc), included by bb_tree.hip after pregrow / Job: its work
// area in HBM and launch plan, the decision whether a launch is its own (sys_take_over), the launch (sys_launch), what follows
// a launch (sys_after_launch: ids into the sequential engines' order, bbh_tree_sys_counts, diagnostics) and its internal error
// with the wait-state dump (sys_internal_error).  run_insert_multi calls those four and touches nothing of bbh_tree::sys itself.
// ---- the level-systolic kernel's work area and launch plan (bb_tree_sys.inc) --------------------------------------------
// the words workgroups talk through: uncached device memory (bb_tree_sys.inc, "Memory model")
static bool sys_mem_host() { return tree_env().sys_mem == 'h'; }
template <typename T>
static hipError_t sys_alloc_uc(T** p, size_t bytes) {
    if (sys_mem_host()) {  // (experiment: pinned host memory, coherent by construction, every access crosses the fabric)
        hipError_t eh = hipHostMalloc((void**)p, bytes, hipHostMallocCoherent);
        return eh;
    }
    // (experiments: "plain" = ordinary device memory, "fine" = fine-grained)
    const char m = tree_env().sys_mem;
    const unsigned flags = m == 'p' ? hipDeviceMallocDefault : (m == 'f' ? hipDeviceMallocFinegrained : hipDeviceMallocUncached);
    hipError_t e = hipExtMallocWithFlags((void**)p, bytes, flags);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        bb::dev_trim();
        e = hipExtMallocWithFlags((void**)p, bytes, flags);
    }
    return e;
}
static void sys_free_uc(void* q) {  // a block of sys_alloc_uc (never cached)
    if (q) (void)(sys_mem_host() ? hipHostFree(q) : hipFree(q));
}
void sys_free(bbh_tree* t) {
    for (void* q : {(void*)t->sys.rings, (void*)t->sys.mail, (void*)t->sys.ctl}) sys_free_uc(q);
    for (void* q : {(void*)t->sys.laste, (void*)t->sys.busy, (void*)t->sys.sent, (void*)t->sys.up, (void*)t->sys.acks}) bb::dev_free(q);
    t->sys = SysDev{};
    t->sys_ring_bytes = 0;
    t->sys_cap_nodes = 0;
    t->sys_G_alloc = 0;
}

// BBHIP_SYS: unset / "0" never (the default: the kernel is OPT-IN), "1" whenever the tree's shape allows it, "auto": where
// the other kernels are weakest (sys_take_over).  Opt-in because its cross-workgroup hand-over is not
// yet dependable on this hardware: the 1 M-row workloads it was built for are per-element identical to the oracle in every one
// of ~100 runs, but the randomised suite's adversarial shapes at bf 254 (every node full, four levels, a split every few
// elements) end in a detected inconsistency or - rarely - a silently different tree in 2-7 % of runs
// (profiles/r06/sys_stability.txt, DESIGN.md 6s).  Read on every call: tests switch it inside one process.
static int sys_mode() {
    const char* v = env_value("BBHIP_SYS");
    return v == nullptr ? 0 : (std::strcmp(v, "auto") == 0 ? 2 : 1);
}

// Are the root's centroids informative (some row's popcount non-zero)?  Trees over sparse / weakly clustered rows keep
// all-zero centroids in their upper levels (every similarity 0, np.argmax -> row 0): one exact level, the shape the pipelined
// kernel was built for (S-fake: 460 k/s there, 274 k/s here).  Trees over real-fingerprint-like rows compare at every level:
// that is what the systolic kernel is for (zipf / hier: 122-131 k/s there, 357-379 k/s here).  Two small blocking copies, made
// only when the pipelined kernel has just handed the tree over.
static bool sys_root_informative(bbh_tree* t) {
    const TreeDev& h = t->h;
    const uint32_t root = h.ctr[C_ROOT];
    NodeHdr hd{};
    if (hipMemcpy(&hd, h.node_hdr + root, sizeof(hd), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return false; }
    const uint32_t len = std::min<uint32_t>(hd.len, (uint32_t)h.bf + 1);
    if (len == 0 || (hd.leaf & HW_LEAF)) return false;
    std::vector<uint32_t> cards(len);
    if (hipMemcpy(cards.data(), h.node_card + (size_t)root * NG, (size_t)len * 4, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return false; }
    for (uint32_t cd : cards)
        if (cd != 0) return true;
    return false;
}

// workgroups per tree level: level 0 is workgroup 0 (the root), the last level the leaf owners
static void sys_plan(const TreeDev& h, SysDev& S) {
    const int levels = (int)h.ctr[C_DEPTH];  // (1: the root is a leaf)
    S.levels = levels;
    int first = 0;
    const int env_int = tree_env().sys_internal_wgs, env_leaf = tree_env().sys_leaf_wgs;
    for (int l = 0; l < levels && l < SYS_MAXLVL; ++l) {
        int cnt;
        if (l == 0) cnt = 1;
        else if (l == levels - 1) cnt = env_leaf > 0 ? env_leaf : 64;
        else cnt = env_int > 0 ? env_int : (h.bf >= 128 ? 64 : 16);  // (bf 254: one mirrored node per owner - as many owners as a level has nodes)
        cnt = std::min(cnt, SYS_MAXPROD);
        while (cnt & (cnt - 1)) cnt &= cnt - 1;  // a power of two (sys_owner_idx)
        S.lvl_first[l] = first;
        S.lvl_count[l] = cnt;
        first += cnt;
    }
    S.G = first;
    // every workgroup has to be RESIDENT (one per CU: the kernel takes most of a CU's LDS) - a workgroup that waits for a CU while
    // the others wait for its answers is a deadlock (found by the randomised suite: five levels at bf 254 came to 257 workgroups)
    while (S.G > 224) {
        first = 0;
        for (int l = 0; l < levels && l < SYS_MAXLVL; ++l) {
            if (l > 0 && l < levels - 1 && S.lvl_count[l] > 8) S.lvl_count[l] /= 2;
            S.lvl_first[l] = first;
            first += S.lvl_count[l];
        }
        if (first == S.G) break;
        S.G = first;
    }
    S.qmax = 384;  // (< SYS_R: no ring can overflow)
}

// (re)allocate what the plan and the node pool's size need; zero the rings and control words, initialise the mailboxes
static int sys_prepare(bbh_tree* t, hipStream_t s) {
    TreeDev& h = t->h;
    SysDev& S = t->sys;
    sys_plan(h, S);
    {
        // the kernel admits an element only while the pools hold the worst case of everything in flight (every element splits
        // every level and the root): make sure a launch starts with that reserve and room to work in
        const uint64_t q = (uint64_t)S.qmax + 64, depth = h.ctr[C_DEPTH], nblk = node_blocks((uint32_t)h.bf + 1);
        const uint64_t room = tiny_pools() ? 16 : 4096;  // (elements' worth of room beyond the reserve)
        BB_TRY(grow_nodes(t, clamp30((uint64_t)h.ctr[C_NODES] + (q * (depth + 2) + room / 8 + 8) * nblk)));
        BB_TRY(grow_cf(t, 0, clamp30((uint64_t)h.ctr[C_N8] + q + room)));
        BB_TRY(grow_cf(t, 1, clamp30((uint64_t)h.ctr[C_N16] + q + 64)));
        BB_TRY(grow_cf(t, 2, clamp30((uint64_t)h.ctr[C_N32] + q * 2 * (depth + 2) + room / 4 + 16)));
    }
    const size_t ring_bytes = (size_t)S.G * SYS_MAXPROD * (size_t)SYS_R * 16;
    {
        static std::atomic<uint32_t> g_sys_launch{0};  // (process-wide: a new tree may inherit another tree's ring memory)
        S.launch_id = (g_sys_launch.fetch_add(1u) + 1u) & 0x7FFFFFFFu;
        if (S.launch_id == 0) S.launch_id = (g_sys_launch.fetch_add(1u) + 1u) & 0x7FFFFFFFu;
    }
    if (ring_bytes > t->sys_ring_bytes || S.G > t->sys_G_alloc) {
        sys_free_uc(S.rings);
        bb::dev_free(S.busy);
        S.rings = nullptr; S.busy = nullptr;
        t->sys_ring_bytes = 0; t->sys_G_alloc = 0;  // (nothing is held until both allocations have succeeded)
        BB_HIP(sys_alloc_uc(&S.rings, ring_bytes));
        BB_HIP(bb::dev_alloc(&S.busy, (size_t)S.G * (15 * 8 + 3 * SYS_MAXPROD * 4) + 64));
        t->sys_ring_bytes = ring_bytes;
        t->sys_G_alloc = S.G;
    }
    if (!S.ctl) BB_HIP(sys_alloc_uc(&S.ctl, SC_COUNT * 4));
    if (h.cap_nodes > t->sys_cap_nodes || !S.mail) {
        sys_free_uc(S.mail);
        bb::dev_free(S.sent); bb::dev_free(S.up); bb::dev_free(S.laste); bb::dev_free(S.acks);
        S.mail = nullptr; S.sent = nullptr; S.up = nullptr; S.laste = nullptr; S.acks = nullptr;
        t->sys_cap_nodes = 0;
        BB_HIP(bb::dev_alloc(&S.laste, (size_t)h.cap_nodes * 4 + 64));
        BB_HIP(bb::dev_alloc(&S.acks, (size_t)h.cap_nodes * 4 + 64));
        BB_HIP(bb::dev_alloc(&S.sent, (size_t)h.cap_nodes * 4 + 64));
        BB_HIP(bb::dev_alloc(&S.up, (size_t)h.cap_nodes * 8 + 64));
        BB_HIP(sys_alloc_uc(&S.mail, (size_t)h.cap_nodes * 8 + 64));
        t->sys_cap_nodes = h.cap_nodes;
    }
    BB_HIP(hipMemsetAsync(S.rings, 0, ring_bytes, s));
    BB_HIP(hipMemsetAsync(S.ctl, 0, SC_COUNT * 4, s));
    BB_HIP(hipMemsetAsync(S.busy, 0, (size_t)S.G * (15 * 8 + 3 * SYS_MAXPROD * 4), s));
    const uint32_t used = std::min(h.cap_nodes, h.ctr[C_NODES]);
    hipLaunchKernelGGL(k_sys_init, dim3((used + 255) / 256), dim3(256), 0, s, (const NodeHdr*)h.node_hdr, used, S.mail, S.sent, S.up, S.laste, S.acks);
    BB_HIP(hipGetLastError());
    return BBH_OK;
}

// ids handed out by a launch of the systolic kernel, renumbered into the sequential engines' order (bb_tree_sys.inc)
static int sys_renumber(bbh_tree* t, uint32_t* out_leaf, uint32_t n, uint32_t base, uint32_t nnew, hipStream_t s) {
    if (out_leaf == nullptr || n == 0 || nnew == 0) return BBH_OK;
    bb::DevScope tmp(s);
    uint32_t *creator = nullptr, *flag = nullptr, *rank = nullptr, *map = nullptr;
    void* d_tmp = nullptr;
    BB_HIP(tmp.get(&creator, (size_t)nnew * 4 + 64));
    BB_HIP(tmp.get(&flag, (size_t)n * 4 + 64));
    BB_HIP(tmp.get(&rank, (size_t)n * 4 + 64));
    BB_HIP(tmp.get(&map, (size_t)nnew * 4 + 64));
    BB_HIP(hipMemsetAsync(creator, 0xFF, (size_t)nnew * 4, s));
    const dim3 ge((n + 255) / 256), gi((nnew + 255) / 256), blk(256);
    hipLaunchKernelGGL(k_sys_creator, ge, blk, 0, s, (const uint32_t*)out_leaf, n, base, creator);
    hipLaunchKernelGGL(k_sys_flag, ge, blk, 0, s, (const uint32_t*)out_leaf, n, base, (const uint32_t*)creator, flag);
    size_t tmp_bytes = 0;
    BB_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, flag, rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
    BB_HIP(tmp.get(&d_tmp, tmp_bytes + 16));
    BB_HIP(rocprim::exclusive_scan(d_tmp, tmp_bytes, flag, rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_sys_map, gi, blk, 0, s, (const uint32_t*)creator, (const uint32_t*)rank, nnew, base, map);
    hipLaunchKernelGGL(k_sys_apply_out, ge, blk, 0, s, out_leaf, n, base, nnew, (const uint32_t*)map);
    const uint32_t used = std::min(t->h.cap_nodes, t->h.ctr[C_NODES]);
    hipLaunchKernelGGL(k_sys_apply_rows, dim3((used + 3) / 4), blk, 0, s, (const NodeHdr*)t->h.node_hdr, t->h.node_rm, used, base, nnew, (const uint32_t*)map);
    BB_HIP(hipGetLastError());
    return tmp.sync();
}
// ---- the kernel's instances ------------------------------------------------------------------------------------------------
struct SysKernel {
    int bf;
    bool phases;  // the phase-timer instance (BBHIP_SYS_PHASES)
    void (*fn)(TreeDev*, SysDev);
    uint32_t lds;
};
#define BB_SYS_ENTRY(KS, BF, PH) {BF, PH, k_tree_sys<KS, PH>, (uint32_t)(KS::o.total + sys_lds_bytes<KS>())}
static const SysKernel kSysKernels[] = {BB_SYS_ENTRY(KS50, 50, false), BB_SYS_ENTRY(KS254, 254, false), BB_SYS_ENTRY(KS50, 50, true), BB_SYS_ENTRY(KS254, 254, true)};
#undef BB_SYS_ENTRY

// (configure: dynamic LDS above 48 KiB has to be allowed per kernel)
static int sys_allow_lds() {
    for (const SysKernel& k : kSysKernels) BB_HIP(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));
    return BBH_OK;
}

// the launch that sys_take_over prepared: as many workgroups as the plan has owners
static void sys_launch(const bbh_tree* t, TreeDev* dptr, hipStream_t s) {
    for (const SysKernel& k : kSysKernels)
        if (k.bf == t->h.bf && k.phases == tree_env().sys_phases) {
            hipLaunchKernelGGL(k.fn, dim3((unsigned)t->sys.G), dim3(TB), k.lds, s, dptr, t->sys);
            return;
        }
}

// Is this launch the level-systolic kernel's?  ONE tree (`sj`, the call's only job, which the steady-state entry `fk` would
// otherwise run) over many workgroups.  BBHIP_SYS=1: whenever the shape allows; "auto": where the pipelined kernel has
// nothing to offer - it asked for its multi-level instance (informative levels above the leaf-parents at bf 50) or refused
// the shape (bf 254) and the steady-state kernel would take the stretch.  If so the tree is prepared (sys_prepare: its pools
// may grow) and *n is the number of elements the launch takes; otherwise *n stays 0.
static int sys_take_over(Job& sj, const FastKernel& fk, hipStream_t s, int64_t* n) {
    const TreeEnv& env = tree_env();
    const int mode = sys_mode();
    // (diagnostics of the pipelined kernel keep it in charge; a call without `out` could not have its ids renumbered - sys_renumber)
    if (mode == 0 || fk.buffers || env.phases || env.pipe_phases || env.pipe_audit != 0 || sj.out == nullptr) return BBH_OK;
    bbh_tree* st = sj.t;
    const int levels = (int)st->h.ctr[C_DEPTH];
    if (levels < 2 || levels > SYS_MAXLVL || st->gc_runs != 0 || st->h.n_elems >= (1ll << 31) || st->sys_off_left != 0) return BBH_OK;
    if (mode == 1) {
        *n = st->h.n_elems;
    } else {
        if (!st->sys_pref && ((fk.bf == 254 && sj.old_left > 0) || (fk.bf == 50 && st->pipe_ml)) && sys_root_informative(st)) st->sys_pref = true;
        if (!st->sys_pref) return BBH_OK;
        sj.old_left = 0;  // (the stretch the steady-state kernel was to take is this kernel's, and so is the rest of the call)
        *n = sj.n - sj.done;
    }
    st->sys_ids_before = st->h.ctr[C_IDS];
    return sys_prepare(st, s);
}

// BBHIP_SYS_PHASES (phase-timer instance): cycles per element of the internal step: the root's owner, and the busiest owner of every other level
static void sys_print_phases(const bbh_tree* t, long long processed) {
    std::vector<unsigned long long> ph((size_t)t->sys.G * 13);
    if (hipMemcpy(ph.data(), t->sys.busy, ph.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return; }
    static const char* names[12] = {"lookup", "compare(hit)", "fill+compare(miss)", "guard", "send", "commit", "rest", "misses", "mailbox-rereads", "reread-spins", "ALONE", "ALONE-wait-cycles"};
    for (int l = 0; l < t->sys.levels; ++l) {
        int best = t->sys.lvl_first[l];
        for (int w = t->sys.lvl_first[l]; w < t->sys.lvl_first[l] + t->sys.lvl_count[l]; ++w)
            if (ph[(size_t)w] > ph[(size_t)best]) best = w;
        fprintf(stderr, "[bbhip sys phases] level %d: %d workgroups, busiest wg %d: busy %.0f cycles per launch element (%lld elements)", l, t->sys.lvl_count[l], best,
                (double)ph[(size_t)best] / (double)processed, processed);
        if (l < t->sys.levels - 1)
            for (int i = 0; i < 12; ++i) fprintf(stderr, " %s %.0f", names[i], (double)ph[(size_t)t->sys.G + (size_t)best * 12 + i] / ((i >= 7 && i <= 10) ? 1.0 : (double)processed));
        fprintf(stderr, "\n");
    }
}

// after a launch of the systolic kernel (`back`: the tree as read back; t->h already holds its counters): ids into the
// sequential engines' order, the record for bbh_tree_sys_counts, the diagnostics
static int sys_after_launch(bbh_tree* t, const TreeDev& back, hipStream_t s) {
    // (ids in the sequential engines' order: bb_tree_sys.inc, "BitFeature ids in the reference's order")
    if (back.stop_reason != STOP_INTERNAL && back.ctr[C_IDS] > t->sys_ids_before)
        BB_TRY(sys_renumber(t, back.out_leaf, (uint32_t)back.processed, t->sys_ids_before, back.ctr[C_IDS] - t->sys_ids_before, s));
    t->syscount[0] += (uint64_t)back.processed;
    t->syscount[1] += 1;
    if (back.stop_reason == STOP_SYS_RELAUNCH) t->syscount[2] += 1;
    t->syscount[3] = (uint64_t)t->sys.G;
    std::vector<unsigned long long> busy((size_t)t->sys.G);
    if (hipMemcpy(busy.data(), t->sys.busy, busy.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
        for (unsigned long long b : busy) t->syscount[4] += b;
        t->syscount[5] += busy[0];
        unsigned long long mx = 0;
        for (size_t q = 1; q < busy.size(); ++q) mx = std::max(mx, busy[q]);
        t->syscount[6] += mx;
    } else {
        (void)hipGetLastError();
    }
    if (back.stop_reason == STOP_SYS_UNSUPPORTED) t->syscount[7] += 1;
    uint32_t stale = 0;
    if (tree_env().sys_debug && hipMemcpy(&stale, t->sys.ctl + SC_STALE_CTL, 4, hipMemcpyDeviceToHost) == hipSuccess && stale != 0)
        fprintf(stderr, "[bbhip sys state] launch %u: %u polls saw a control word that a read-modify-write read did not, %u saw another launch's FINISH\n", t->sys.launch_id, stale & 0xFFFFu, stale >> 16);
    if (tree_env().sys_phases && back.processed > 0) sys_print_phases(t, (long long)back.processed);
    return BBH_OK;
}

// ---- BBHIP_SYS_DEBUG: where every workgroup was waiting when the kernel gave up ---------------------------------------------
// the words a wait is about, as the host sees them now
static void sys_dump_words(const bbh_tree* t, uint32_t nd, const char* what) {
    unsigned long long mw = 0, upw = 0; uint32_t sw = 0, le = 0; NodeHdr hd{};
    if (nd >= t->h.cap_nodes) return;
    (void)hipMemcpy(&mw, t->sys.mail + nd, 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&upw, t->sys.up + nd, 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&sw, t->sys.sent + nd, 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&le, t->sys.laste + nd, 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&hd, t->h.node_hdr + nd, sizeof(hd), hipMemcpyDeviceToHost);
    fprintf(stderr, "[bbhip sys state]     %s %u: mail acked %u len %u res %u epoch %u | sent %u | last element+1 %u | up (node %u row %u) | hdr len %u leaf %#x\n", what, nd,
            (unsigned)mw, (unsigned)((mw >> 32) & 0xFFFF), (unsigned)((mw >> 48) & 3), (unsigned)(mw >> 50), sw, le, (unsigned)(upw >> 32), (unsigned)upw, hd.len, hd.leaf);
}

// one workgroup that waited in a guard / ALONE / drain on node `nd` for child `ch`: their words, where the tree (as the host
// sees it now) holds the child and the node's first rows, and (drain) the children that are behind
static void sys_dump_wait(const bbh_tree* t, unsigned kind, uint32_t nd, uint32_t ch) {
    sys_dump_words(t, nd, "node");
    sys_dump_words(t, ch, "child");
    const uint32_t used = std::min<uint32_t>(t->h.cap_nodes, 1u << 22), nblk = node_blocks((uint32_t)t->h.bf + 1);
    std::vector<uint32_t> lk((size_t)used * NG);
    std::vector<NodeHdr> hh(used);
    if (hipMemcpy(lk.data(), t->h.node_link, lk.size() * 4, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(hh.data(), t->h.node_hdr, hh.size() * sizeof(NodeHdr), hipMemcpyDeviceToHost) == hipSuccess) {
        if (nd < used) {
            fprintf(stderr, "[bbhip sys state]     node %u rows' children:", nd);
            for (uint32_t r = 0; r < hh[nd].len && r < 6; ++r) fprintf(stderr, " %u", lk[(size_t)nd * NG + r]);
            fprintf(stderr, "\n");
        }
        for (uint32_t x = 0; x + nblk <= used; ++x) {
            if ((hh[x].leaf & HW_LEAF) || hh[x].len == 0 || hh[x].len > (uint32_t)t->h.bf + 1 || hw_cap(hh[x].leaf) != (uint32_t)t->h.bf + 1) continue;
            for (uint32_t r = 0; r < hh[x].len; ++r)
                if (lk[(size_t)x * NG + r] == ch) fprintf(stderr, "[bbhip sys state]     child %u is row %u of node %u (len %u)\n", ch, r, x, hh[x].len);
        }
    }
    if (kind != 3) return;
    NodeHdr hd{};
    (void)hipMemcpy(&hd, t->h.node_hdr + nd, sizeof(hd), hipMemcpyDeviceToHost);
    for (uint32_t r = 0; r < hd.len && r <= (uint32_t)t->h.bf; ++r) {
        uint32_t c = 0, sw = 0; unsigned long long mw = 0;
        (void)hipMemcpy(&c, t->h.node_link + (size_t)nd * NG + r, 4, hipMemcpyDeviceToHost);
        if (c >= t->h.cap_nodes) continue;
        (void)hipMemcpy(&sw, t->sys.sent + c, 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(&mw, t->sys.mail + c, 8, hipMemcpyDeviceToHost);
        if ((uint32_t)mw != sw) sys_dump_words(t, c, "  behind: row's child");
    }
}

// ring positions: what a producer sent and its consumer has not taken
static void sys_dump_rings(const bbh_tree* t) {
    std::vector<uint32_t> pos((size_t)t->sys.G * 2 * SYS_MAXPROD);
    if (hipMemcpy(pos.data(), (const uint8_t*)t->sys.busy + (size_t)t->sys.G * 15 * 8, pos.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
    for (int l = 0; l + 1 < t->sys.levels; ++l)
        for (int p = 0; p < t->sys.lvl_count[l]; ++p)
            for (int q = 0; q < t->sys.lvl_count[l + 1]; ++q) {
                const int pw = t->sys.lvl_first[l] + p, cw = t->sys.lvl_first[l + 1] + q;
                const uint32_t tail = pos[(size_t)pw * 2 * SYS_MAXPROD + SYS_MAXPROD + q], head = pos[(size_t)cw * 2 * SYS_MAXPROD + p];
                if (tail == head) continue;
                unsigned long long ab[2] = {0, 0};
                (void)hipMemcpy(ab, t->sys.rings + (((size_t)cw * SYS_MAXPROD + (size_t)p) * SYS_R + (head & (SYS_R - 1u))) * 2, 16, hipMemcpyDeviceToHost);
                fprintf(stderr, "[bbhip sys state] ring wg %d -> wg %d: sent %u taken %u; the slot the consumer is looking at: %016llx %016llx (launch id %u: gen %u alone %u node %u element %u | gen %u launch %u epoch %u)\n",
                        pw, cw, tail, head, ab[0], ab[1], t->sys.launch_id, (unsigned)(ab[0] >> 63), (unsigned)((ab[0] >> 62) & 1), (unsigned)((ab[0] >> 31) & 0x3FFFFFFF),
                        (unsigned)(ab[0] & 0x7FFFFFFF), (unsigned)(ab[1] >> 63), (unsigned)((ab[1] >> 32) & 0x7FFFFFFF), (unsigned)ab[1]);
            }
}

// STOP_INTERNAL of a systolic launch: the error, and under BBHIP_SYS_DEBUG the wait-state dump
static int sys_internal_error(const bbh_tree* t, const TreeDev& back) {
    uint32_t dbg[16] = {0};
    (void)hipMemcpy(dbg, t->sys.ctl, sizeof(dbg), hipMemcpyDeviceToHost);
    const int rc = bb::fail(BBH_ERR_HIP, "level-systolic kernel: internal error at bb_tree_sys.inc:%u (node %u child %u sent %u acked %u | fresh sent %u acked %u | level/miss/row %#x element %u)",
                            back.giveup_line, dbg[8], dbg[9], dbg[10], dbg[11], dbg[12], dbg[13], dbg[14], dbg[15]);
    std::vector<unsigned long long> stw((size_t)t->sys.G * 15);
    if (!tree_env().sys_debug || hipMemcpy(stw.data(), t->sys.busy, stw.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return rc;
    for (int w = 0; w < t->sys.G; ++w) {
        const unsigned long long a = stw[(size_t)t->sys.G * 13 + (size_t)w * 2], b = stw[(size_t)t->sys.G * 13 + (size_t)w * 2 + 1];
        const unsigned kind = (unsigned)(a >> 32);
        if (kind != 4)
            fprintf(stderr, "[bbhip sys state] wg %d: %s node %u child %u want %u (owner index of child in the next level: %u)\n", w,
                    kind == 1 ? "guard (pending below the child)" : kind == 2 ? "ALONE (waits for the child)" : kind == 3 ? "drain (all children)" : kind == 5 ? "in an internal step (node, element, alone)" : kind == 6 ? "in a leaf step (node, element, alone)" : "busy / never polled",
                    (unsigned)a, (unsigned)(b >> 32), (unsigned)b, (unsigned)(((unsigned)(b >> 32)) / node_blocks((uint32_t)t->h.bf + 1)));
        if (kind >= 1 && kind <= 3) sys_dump_wait(t, kind, (uint32_t)a, (uint32_t)(b >> 32));
    }
    sys_dump_rings(t);
    for (int l = 0; l < t->sys.levels; ++l) fprintf(stderr, "[bbhip sys state] level %d: workgroups %d..%d\n", l, t->sys.lvl_first[l], t->sys.lvl_first[l] + t->sys.lvl_count[l] - 1);
    return rc;
}
