// bb_tree_route.inc -- route fingerprints through a fitted tree WITHOUT inserting them (bbh_tree_route_packed; DESIGN.md
// section 5g).
//
// The read-only twin of the insertion kernels: for every query row, what _BFNode.insert_bf_subcluster (bitbirch.py:305-357)
// does up to, but not including, its first write - the greedy descent by first argmax of the exact Tanimoto fraction, then
// the merge test of the chosen leaf row against the query as a one-fingerprint nominee.  Nothing of the tree is written: no
// node is thawed (a sealed node is read where it lies: node_best masks rows >= len and the pools end in a pad of bf + 1
// rows, "Node storage" in bb_tree.hip), no counter moves, no pool grows.
//
// A frozen tree has no dependency between queries, so the mapping is the plainest one: ONE WORKGROUP OF FOUR WAVES PER
// QUERY, workgroups striding over the queries, no workgroup ever waiting for another.  Every stage is the insertion
// kernels' own device function on the run-time-shape context (bf 2..1023, 8..8192 bits, one code path per row width as
// there): node_best for a level (all four waves on one node: 16 lanes x 16 B per row, 16 rows per pass, cand_better for
// the exact first argmax), cf_load8 with the tier decoding for the leaf row's linear sum, block_sum for the dot product,
// merge_accept (isim_from_moments, radius_terms, radius_compl, tol_lookup) for the decision - the same float64 operations
// in the same order as an insertion would perform.  The LDS a workgroup needs is the query row, the double-buffered link
// words of one node and two reduction buffers (route_layout: 1.2 KB at bf 50 x 2048 bits, 9.5 KB at bf 1023 x 8192 bits),
// so registers, not LDS, set the residency: 124 VGPRs, four workgroups (16 waves) per CU, which hide each other's memory
// round trips; the upper levels are shared by all queries and stay in L2.
//
// Corruption never becomes a loop or an out-of-pool read: the walk visits at most the tree's recorded depth (<= MAXD)
// levels, a child link is checked against cap_nodes and a cluster-feature slot against its pool before it is followed, a
// node without rows ends the walk; the query's workgroup then raises the call's error word and stops.
#if defined(__HIPCC__)

constexpr unsigned ROUTE_GRID_MAX = 256 * 8;  // workgroups of a launch (two rounds of the resident ones); beyond that a workgroup takes several queries

// the insertion context without the BitFeature-buffer path: a query is a packed fingerprint
using KCRoute = KCWith<KC, 0>;

// LDS of a routing workgroup: only what node_best (without counts, without mirrors), elem_cols and block_sum touch
__host__ __device__ constexpr Smem route_layout(int bf, int RB) {
    Smem s{};
    SmemCursor c;
    const size_t m = (size_t)bf + 1;
    s.x = c.take(RB);
    s.vec = s.x;
    s.link = c.take(2 * m * 4);
    s.red = c.take(2 * TW * NRED * 8);
    s.wbest = c.take(2 * TW * 8);
    s.total = c.off;
    return s;
}

__global__ __launch_bounds__(TB) void k_tree_route(const TreeDev T, const uint8_t* __restrict__ in_rows, long long row_stride, long long n,
                                                   uint32_t* __restrict__ out_leaf, uint8_t* __restrict__ out_accept,
                                                   uint32_t* __restrict__ out_inter, uint32_t* __restrict__ out_union, uint32_t* err) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    KCRoute k;
    k.cent = T.node_cent; k.card = T.node_card; k.link = T.node_link; k.rm = T.node_rm; k.hdr = T.node_hdr;
    k.scratch = nullptr; k.cf8 = T.cf8; k.cf16 = T.cf16; k.cf32 = T.cf32;
    k.bufs = nullptr; k.width = 0;
    k.crit = T.crit; k.tol_len = T.tol_len; k.thr = T.thr; k.tolerance = T.tolerance; k.tol = T.tol_table;
    k.L = (LA unsigned char*)smem_raw;
    k.F = T.F; k.nb = T.nbytes; k.RB = T.RB; k.RBc = k.RB / 16; k.RBS = k.RB + 16;
    k.bf = (uint32_t)T.bf; k.rows = k.bf + 1; k.nblk = node_blocks(k.rows);
    k.nm = 0;
    k.o = route_layout((int)k.bf, k.RB);
    const int tid = threadIdx.x;
    const int nb = k.nb;
    const uint32_t root = T.ctr[C_ROOT];
    const uint32_t max_levels = T.ctr[C_DEPTH] < (uint32_t)MAXD ? T.ctr[C_DEPTH] : (uint32_t)MAXD;
    const uint32_t cap_nodes = T.cap_nodes;
    LA u32x4_t* sx = lds<u32x4_t>(k.L, k.o.x);
    int red_slot = 0, cmp_par = 0;
    for (long long e = blockIdx.x; e < n; e += gridDim.x) {
        __syncthreads();  // (the previous query's row and link words have been read by everyone)
        // ---- the query row into LDS, padding bytes zero
        const uint8_t* row = in_rows + e * row_stride;
        if ((((uintptr_t)row) & 15) == 0 && (nb & 15) == 0) {
            for (int ch = tid; ch < k.RBc; ch += TB) sx[ch] = ldg<u32x4_t>(row + (size_t)ch * 16);
        } else {
            for (int b = tid; b < k.RB; b += TB) lds<uint8_t>(k.L, k.o.x)[b] = b < nb ? ldg<uint8_t>(row + b) : (uint8_t)0;
        }
        __syncthreads();
        Elem el;
        el.idx = e;
        el.nS = 1;
        el.pcx = uni(lds_vec_popcount(k, k.o.x));
        el.s1S = el.pcx;
        el.s2S = el.pcx;

        // ---- greedy descent (bitbirch.py:305-320), bounded by the recorded depth
        uint32_t nd = uni(root < cap_nodes ? root : NONE), j = 0, link = NONE, leaf = 0, level = 0;
        bool bad = nd == NONE;
        Cand best{0, 1, NONE};
        while (!bad) {
            nd = uni(nd);
            level = uni(level);
            uint32_t len = 0, leafw = 0;
            best = node_best<false, false>(k, cmp_par, nd, -1, k.o.x, el.pcx, false, false, true, &len, &leafw);
            j = uni(best.r);
            if (j >= k.rows) { bad = true; break; }  // (a node without rows: NONE)
            link = uni(lds<uint32_t>(k.L, k.o.link)[cmp_par * k.rows + j]);
            leaf = uni(leafw & HW_LEAF);
            if (leaf) break;
            if (level + 1 >= max_levels || link >= cap_nodes) { bad = true; break; }
            nd = link;
            level++;
        }
        // ---- the chosen leaf row: its record, its cluster features, the merge test (bitbirch.py:321-326)
        uint32_t Tsub = NONE, card = 0;
        bool accept = false;
        if (!bad) {
            const size_t m = (size_t)nd * NG + j;
            const uint8_t* rmp = (const uint8_t*)(k.rm + m);
            const u32x4_t rm0 = ldg<u32x4_t>(rmp), rm1 = ldg<u32x4_t>(rmp + 16);
            card = uni(ldg<uint32_t>(k.card + m));
            Tsub = uni(rm0.x);
            const u64 nT = uni(rm0.y);
            const u64 s1T = ((u64)uni(rm1.y) << 32) | uni(rm1.x);
            const u64 s2T = ((u64)uni(rm1.w) << 32) | uni(rm1.z);
            const uint32_t slotT = link;  // leaf row: link = CF slot word
            const uint32_t slotE = slot_effective(slotT, nT);  // (one member: the centroid row is the linear sum)
            const uint32_t tierE = slotE >> 30, idxE = slotE & 0x3FFFFFFFu;
            const uint32_t capE = tierE == 0 ? T.cap8 : (tierE == 1 ? T.cap16 : (tierE == 2 ? T.cap32 : 0xFFFFFFFFu));
            const u64 new_n = nT + 1;
            if (idxE >= capE) {
                bad = true;
            } else if (new_n <= 0xFFFFFFFFull) {  // (an insertion would stop with STOP_RANGE: no merge)
                const uint8_t* const crow = k.cent + m * (size_t)k.RB;
                u64 dot[1] = {0};
                for (int b = tid; b < nb; b += TB) {
                    uint32_t v[8], x8[8];
                    cf_load8(k, slotE, b, v, crow);
                    elem_cols(k, el, b, x8);
#pragma unroll
                    for (int q = 0; q < 8; ++q) dot[0] += (u64)v[q] * x8[q];
                }
                block_sum<1>(k, red_slot, dot);
                const u64 s1n = s1T + el.s1S;
                const u64 s2n = s2T + 2ull * dot[0] + el.s2S;
                accept = merge_accept(k, el, red_slot, slotE, crow, nT, s1T, s2T, new_n, s1n, s2n);
            }
        }
        if (bad) {
            if (tid == 0) atomicOr(err, 1u);
            break;
        }
        if (tid == 0) {
            if (out_leaf) out_leaf[e] = Tsub;
            if (out_accept) out_accept[e] = accept ? 1 : 0;
            if (out_inter) out_inter[e] = best.i;
            if (out_union) out_union[e] = card + el.pcx - best.i;  // (the true union: 0 for two empty rows)
        }
    }
}

#endif  // __HIPCC__
