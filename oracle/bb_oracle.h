/*
 * bb_oracle.h -- CPU restatement ("oracle") of the BitBIRCH similarity / insertion hot
 * path of mqcomplab/bblean.  TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's `cpu_baseline` leg may load this
 * library.  The product (bblean_amd + libbbhip.so) never links, imports or calls it.
 *
 * Parity status: PINNED.  Every function is checked (tests/test_oracle_golden.py)
 * against fixtures under tests/golden/ that were produced by importing the reference
 * itself (tests/golden/make_golden.py) and against the known-answer values the
 * reference's own tests hold (tests/test_similarity.py, test_refine.py,
 * test_bb_consistency.py, test_multiround.py, test_merges.py of the reference).
 *
 * Each function cites the reference lines it restates, relative to /root/reference/.
 */
#ifndef BB_ORACLE_H
#define BB_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* merge criteria, bblean/_merges.py:194-212 */
enum {
    BBO_CRIT_DIAMETER = 0,      /* _merges.py:56-69   */
    BBO_CRIT_RADIUS = 1,        /* _merges.py:40-53   */
    BBO_CRIT_TOL_DIAMETER = 2,  /* _merges.py:72-116  */
    BBO_CRIT_TOL_RADIUS = 3,    /* _merges.py:119-142 */
    BBO_CRIT_TOL_LEGACY = 4,    /* _merges.py:164-191 */
    BBO_CRIT_NEVER = 5          /* _merges.py:145-161 */
};

/* ---- stateless kernels (bblean/csrc/similarity.cpp) ------------------------------ */

/* _popcount_2d, similarity.cpp:99-141 */
void bbo_popcount_rows(const uint8_t* arr, int64_t n, int64_t nbytes, uint32_t* out);
/* _calc_arr_vec_jt + jt_sim_packed_precalc_cardinalities, similarity.cpp:304-372.
 * card may be NULL (then computed like _jt_sim_arr_vec_packed, :374-377). */
void bbo_jt_arr_vec(const uint8_t* arr, int64_t n, int64_t nbytes, const uint8_t* vec,
                    const uint32_t* card, double* out_sim, uint32_t* out_inter,
                    uint32_t* out_union);
/* unpack_fingerprints, similarity.cpp:145-214 (MSB first; n_features % 8 == 0) */
void bbo_unpack(const uint8_t* packed, int64_t n, int64_t nbytes, int64_t n_features,
                uint8_t* out);
/* np.packbits(axis=-1), fingerprints.py:46-49 */
void bbo_pack(const uint8_t* unpacked, int64_t n, int64_t n_features, uint8_t* out);
/* centroid_from_sum, _py_similarity.py:12-42 and similarity.cpp:216-271.
 * out has n_features bytes if !pack else (n_features+7)/8 bytes. */
void bbo_centroid_from_sum(const uint64_t* ls, int64_t n_features, int64_t n_samples,
                           int pack, uint8_t* out);
/* jt_isim_from_sum, similarity.cpp:273-301; returns NaN when n_objects < 2 */
double bbo_isim_from_sum(const uint64_t* ls, int64_t n_features, int64_t n_objects);
/* add_rows, similarity.cpp:381-400 */
void bbo_add_rows(const uint8_t* arr, int64_t n, int64_t n_features, uint64_t* out);
/* jt_most_dissimilar_packed, similarity.cpp:413-471 */
void bbo_most_dissimilar(const uint8_t* Y, int64_t n, int64_t nbytes, int64_t n_features,
                         int64_t* idx1, int64_t* idx2, double* sims1, double* sims2);
/* jt_isim_radius_compl_from_sum, similarity.py:192-202 */
double bbo_isim_radius_compl_from_sum(const uint64_t* ls, int64_t n_features, int64_t n);
/* one merge decision, _merges.py (whole file). tol_table[old_n] = the reference's
 * max(tolerance*(np.exp(-decay*old_n)-offset),0.0), computed by the caller with numpy
 * (indices >= tol_len mean 0.0). */
int bbo_merge_accept(int crit, double thr, double tolerance, const double* tol_table,
                     int64_t tol_len, const uint64_t* new_ls, int64_t new_n,
                     const uint64_t* old_ls, int64_t old_n, int64_t nom_n,
                     int64_t n_features);

/* ---- stateful tree engine (bblean/bitbirch.py) ------------------------------------- */

typedef struct bbo_tree bbo_tree;

/* BitBirch.__init__, bitbirch.py:596-643 */
bbo_tree* bbo_tree_create(int32_t branching_factor, double threshold, int32_t criterion,
                          double tolerance, const double* tol_table, int64_t tol_len,
                          int32_t n_features);
void bbo_tree_destroy(bbo_tree* t);
/* BitBirch.set_merge, bitbirch.py:674-703 (caller resolves the None-means-keep rules) */
void bbo_tree_set_merge(bbo_tree* t, int32_t criterion, double tolerance,
                        const double* tol_table, int64_t tol_len, double threshold,
                        int32_t branching_factor);
/* BitBirch.reset, bitbirch.py:1078-1090 */
void bbo_tree_reset(bbo_tree* t);
/* BitBirch.fit hot loop, bitbirch.py:769-787.  rows: n x nbytes packed fingerprints.
 * out_leaf[e] = id of the leaf BitFeature element e ended in (merged into or created). */
int bbo_tree_fit_packed(bbo_tree* t, const uint8_t* rows, int64_t n, uint32_t* out_leaf);
/* BitBirch._fit_buffers hot loop, bitbirch.py:848-866.  bufs: k x (n_features+1)
 * elements of `width` bytes (1,2,4,8); last column = n_samples. */
int bbo_tree_fit_buffers(bbo_tree* t, const void* bufs, int32_t width, int64_t k,
                         uint32_t* out_leaf);
/* number of leaf BitFeatures (BitBirch._get_leaf_bfs(sort=False), bitbirch.py:1216) */
int64_t bbo_tree_leaf_count(const bbo_tree* t);
/* leaves in leaf-chain order (bitbirch.py:886-893).  Any output may be NULL.
 * linear_sums: k x n_features uint32. */
void bbo_tree_export_leaves(const bbo_tree* t, uint32_t* leaf_ids, uint64_t* n_samples,
                            uint8_t* packed_centroids, uint32_t* linear_sums);
/* BitFeature buffer rows [linear sum, n_samples] of the leaves at `positions` (indices into that order), `width`
 * (1, 2, 4 or 8) bytes per value; 0 on success. */
int bbo_tree_gather_buffers(const bbo_tree* t, const int64_t* positions, int64_t m, int32_t width, void* out);
/* counters: [0]=similarity calls, [1]=rows compared, [2]=merges, [3]=appends,
 * [4]=splits, [5]=nodes, [6]=max depth seen */
void bbo_tree_stats(const bbo_tree* t, uint64_t* out7);
/* how often the tree sat on an edge, since create or reset; no decision reads them:
 * [0]=merge decisions evaluated (never-merge evaluates none), [1]=those in which a >= or < of the criterion compared two
 * equal float64 values, [2]=best-row searches whose maximum similarity is > 0 and attained by more than one row,
 * [3]=those of [2] whose tied rows have different (intersection, union) pairs */
void bbo_tree_edge_counts(const bbo_tree* t, uint64_t* out4);
/* [3] of the edge counts by the depth of the node that was searched: out8[d - 1] for depth d (the root is 1), the last
 * entry for 8 and deeper.  Depths below the tree's deepest are internal levels. */
void bbo_tree_tie_depths(const bbo_tree* t, uint64_t* out8);
/* what the node splits (_split_node, bitbirch.py:162-211, with jt_most_dissimilar_packed, similarity.cpp:413-471) met on
 * their edges, since create or reset; no decision reads them.  Splits ...
 * [0] in all, [1] of internal nodes, [2] of the root,
 * [3] with a column whose count c over the node's m centroids has 2 * c == m (the majority vote's tie),
 * [4] whose first argmin (similarity to the majority centroid) is attained by more than one row, [5] the same for the second
 *     argmin (similarity to fp1),
 * [6] with a row other than fp1 whose similarities to fp1 and to fp2 are equal, [7] with such a row whose two
 *     (intersection, union) pairs differ,
 * [8] with fp1 == fp2, [9] with n1 == n2, [10] with n1 > n2 (n1: rows that went to the new node, n2: rows that stayed),
 * and, of the SMALLER half (the new node's rows when n1 <= n2, else the rows that stayed; s rows):
 * [11] with a row of n_samples > 255, [12] of n_samples > 65 535, [13] with s % 16 == 0, [14] with s % 16 == 1,
 * [16] all of whose rows have n_samples == 1, [17] whose rows all have n_samples <= 255, some == 1 and some > 1, [18] s > 16;
 * [15] with a row of popcount zero in the node, [19] of a node of more than 124 rows, [20] whose fp1 is row 0, [21] whose fp1
 * is the last row.  [22..23] are zero. */
#define BBO_SPLIT_COUNTS 24
void bbo_tree_split_counts(const bbo_tree* t, uint64_t* out24);
/* The whole tree in pre-order: the root first, then the subtrees of its rows in row order.  Call it with NULL arrays for the
 * counts, then with arrays of that size; any array may be NULL.
 * nodes: n_nodes x 4 int32 [depth (the root is 1), leaf flag, length, position in the leaf chain (-1: an internal node)];
 * per row, the rows of node k after those of node k - 1: n_samples, BitFeature id (0xFFFFFFFF: a tracking row), popcount
 * and packed centroid as the node holds them, linear sum (n_features uint64). */
void bbo_tree_walk(const bbo_tree* t, int64_t* n_nodes, int64_t* n_rows, int32_t* nodes, uint64_t* row_n, uint32_t* row_id,
                   uint32_t* row_popcount, uint8_t* row_centroids, uint64_t* row_linear_sums);


/* ---- the storage model: how the engine keeps its nodes ("Node storage", bblean_amd/csrc/bb_tree.hip) --------------------
 * The reference's node is a Python list; the engine packs nodes in blocks of 4 rows, seals nodes in a compaction and thaws
 * them when an insertion reaches them.  The oracle follows that on its own nodes: per node a recorded length (none, or a
 * value) and a capacity (full, or sealed at ceil(max(len, 1) / 4) blocks).  It only observes: no result of any other call
 * depends on it.  Every sealed node an insertion meets on its way down is thawed, the root first. */
/* gc_nodes (k_gc_size, k_gc_move): a node is cold when `seal` is set, it is not the root, and it is sealed already or its
 * recorded length equals its length; a cold node gets its length rounded up to blocks (full capacity when that is as many
 * blocks), every other node full capacity; every node records its length.  Nothing happens on a tree that never received
 * anything (bbh_tree_compact). */
void bbo_tree_compact(bbo_tree* t, int32_t seal);
/* what bbh_tree_load_fd leaves (k_img_size, k_img_pack): the root full, every other node at its rounded length, every length
 * recorded, the compaction counters those of a fresh handle, the thaw count that of the saved tree. */
void bbo_tree_mark_loaded(bbo_tree* t);
/* [0]=blocks in the used part of the node pools (0: no pools yet), [1]=compactions, [2]=cold nodes and [3]=full nodes of the
 * last one, [4]=thaws since create or reset, [5]=nodes sealed now, [6]=live nodes, [7]=1 once the tree owns pools */
void bbo_tree_storage(const bbo_tree* t, uint64_t* out8);
/* what the thaws met, since create or reset; no decision reads them.  Thaws ...
 * [0] of leaves, [1] of internal nodes, of a leaf that was [2] the first of the chain, [3] the last, [4] neither,
 * [5] of a leaf whose parent the same insertion thawed, [6] of a leaf that then took a merge (no length changes),
 * [7] of a leaf that then took an append, [8] of a leaf / [9] of an internal node that the same insertion then split,
 * [10] insertions that thawed a node and made a new root, [11] those that thawed every node below the root,
 * [12] splits of a leaf that was thawed since the last compaction or load,
 * [13] splits after which the half that stayed in place has exactly its recorded length (it keeps the record),
 * [14] visits of a node other than the root that has a record and full capacity (cold but not sealed: no thaw),
 * [15] of an internal node whose children are leaves, [16] of another internal node directly under the root,
 * [17] of a leaf on level 3 or deeper whose parent was at full capacity already (thawed since the sealing),
 * [18..21] of a leaf of length = 0, 1, 2, 3 (mod 4) that then took an append.  [22], [23] are zero. */
#define BBO_THAW_COUNTS 24
void bbo_tree_thaw_counts(const bbo_tree* t, uint64_t* out24);

#ifdef __cplusplus
}
#endif
#endif
