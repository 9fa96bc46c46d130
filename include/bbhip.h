/*
 * bbhip.h -- C ABI of libbbhip.so, the MI355X (gfx950 / CDNA4) BitBIRCH similarity and
 * insertion engine.  This is the drop-in boundary for the hot path of mqcomplab/bblean:
 * every entry point replaces one binding of the reference's only native module,
 * `bblean._cpp_similarity` (bblean/csrc/similarity.cpp:473-521), or one piece of the
 * per-fingerprint Python loop that calls it (bblean/bitbirch.py:769-787, :848-866).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch/pybind types.
 *   - every data pointer may be a HOST pointer or a DEVICE (hipMalloc / torch) pointer;
 *     the library detects which (hipPointerGetAttributes).  Host inputs are staged to
 *     HBM, host outputs are copied back before the call returns.  With device pointers
 *     the call only enqueues work on `stream` (NULL = the default stream) unless stated.
 *   - return value: 0 on success, non-zero error code otherwise; bbh_last_error() gives
 *     the message for the calling thread.  (The reference throws std::runtime_error,
 *     similarity.cpp:64-66, :345-351; the Python shim maps codes back to RuntimeError /
 *     ValueError / RuntimeWarning.)
 *   - the library never frees or keeps caller memory; `bbh_tree` handles are created and
 *     destroyed explicitly and are not thread-safe.
 *   - packed fingerprints are uint8 rows, most significant bit first (np.packbits,
 *     bblean/fingerprints.py:46), C-contiguous with the given row stride.
 */
#ifndef BBHIP_H
#define BBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBH_OK 0
#define BBH_ERR_INVALID 1     /* bad argument (reference: RuntimeError / ValueError)   */
#define BBH_ERR_HIP 2         /* a HIP runtime call failed                             */
#define BBH_ERR_NO_DEVICE 3   /* no gfx950 device visible                              */
#define BBH_ERR_CAPACITY 4    /* device pools exhausted and could not grow             */
#define BBH_ERR_STATE 5       /* call not valid in the current tree state              */

/* merge criteria, bblean/_merges.py:194-212 */
#define BBH_CRIT_DIAMETER 0
#define BBH_CRIT_RADIUS 1
#define BBH_CRIT_TOL_DIAMETER 2
#define BBH_CRIT_TOL_RADIUS 3
#define BBH_CRIT_TOL_LEGACY 4
#define BBH_CRIT_NEVER 5

const char* bbh_last_error(void);
/* library / device info: writes "gfx950 <name> CUs=.. HBM=.." ; returns device count */
int bbh_device_count(void);
int bbh_device_info(int device, char* buf, size_t buflen);
/* Device blocks released by trees and calls are kept for reuse (hipFree synchronises the device);
 * this returns them to the driver, e.g. before handing the GPU to another allocator.  No
 * reference counterpart: NumPy's allocator plays this role there. */
int bbh_trim_cache(void);

/* A function the library calls when a device allocation fails, before it tries once more: the host side hands over what
 * IT caches on the device (the Python shim registers torch.cuda.empty_cache - a caching tensor allocator keeps freed round
 * tables of gigabytes that the driver then cannot give to a growing tree pool).  NULL removes it. */
int bbh_set_memory_pressure_callback(void (*fn)(void));

/* ---------------------------------------------------------------------------------- */
/* Stateless kernels -- one per pybind11 binding of similarity.cpp:473-521             */
/* ---------------------------------------------------------------------------------- */

/* _popcount_2d (similarity.cpp:99-141) and _popcount_1d (:63-94, n = 1).
 * arr: n rows x nbytes, row_stride bytes apart (>= nbytes); the last row needs only nbytes bytes, so a view that
 * ends where its buffer ends is fine.  out: n uint32. */
int bbh_popcount_rows(const uint8_t* arr, int64_t n, int64_t nbytes, int64_t row_stride,
                      uint32_t* out, void* stream);

/* _jt_sim_arr_vec_packed (similarity.cpp:374-377) = jt_sim_packed_precalc_cardinalities
 * (:340-372) + _calc_arr_vec_jt (:304-333):
 *   out_sim[i] = inter_i / max(double(card_i + popcount(vec) - inter_i), 1.0)
 * card: optional precomputed row popcounts (NULL -> computed in the same pass).
 * arr: rows row_stride bytes apart (>= nbytes); the last row needs only nbytes bytes.
 * out_inter / out_union: optional exact integer numerators / denominators (uint32). */
int bbh_jt_arr_vec(const uint8_t* arr, int64_t n, int64_t nbytes, int64_t row_stride,
                   const uint8_t* vec, const uint32_t* card, double* out_sim,
                   uint32_t* out_inter, uint32_t* out_union, void* stream);

/* Batched best match: for each of nq query rows, the FIRST index of the maximum
 * Tanimoto against nc centroid rows (np.argmax at bitbirch.py:320 fused with the
 * similarity call at :317).  out_idx: nq int32; out_inter/out_union: optional nq uint32
 * of the winning pair; out_sims: optional nq x nc float64 full matrix
 * (jt_sim_matrix_packed, similarity.py:239-247, when queries == centroids).
 * Any nbytes: the comparison is an exact integer cross-multiplication at every row width (64-bit products where
 * the counts need them), never a comparison of rounded quotients. */
int bbh_jt_best_match(const uint8_t* queries, int64_t nq, const uint8_t* cents, int64_t nc,
                      int64_t nbytes, int32_t* out_idx, uint32_t* out_inter,
                      uint32_t* out_union, double* out_sims, void* stream);

/* sklearn.BitBirch.predict's inner step (bblean/sklearn.py:123-137 = pairwise_distances_argmin, metric
 * "jaccard"): out_idx[q] = FIRST index of the minimum of (u - i) / u over the nc centroid rows, distance 0
 * where u == 0 (i = popcount of the AND, u = |q| + |c| - i).  An empty union therefore beats every other pair,
 * which is where this differs from bbh_jt_best_match.  1 <= nc < 2^31; query rows q_stride bytes apart.
 * out_inter / out_union: optional, the winning pair's exact counts (true union, 0 allowed).
 * BBHIP_ASSIGN=bcnt|mfma forces the AND + popcount or the int8 matrix-core kernel (the latter: nbytes == 256,
 * 16-byte aligned rows); unset = chosen by shape.  The result does not depend on the kernel. */
int bbh_jt_assign(const uint8_t* queries, int64_t nq, int64_t q_stride, const uint8_t* cents, int64_t nc,
                  int64_t nbytes, int32_t* out_idx, uint32_t* out_inter, uint32_t* out_union, void* stream);

/* sklearn.BitBirch.transform (sklearn.py:139-153 = pairwise_distances, metric "jaccard"): nq x nc float64,
 * out[q * nc + m] = (u - i) / u as ONE division of the exact integers (not 1 - i / u), 0.0 where u == 0. */
int bbh_jt_dist_matrix(const uint8_t* queries, int64_t nq, int64_t q_stride, const uint8_t* cents, int64_t nc,
                       int64_t nbytes, double* out, void* stream);

/* The k nearest rows of a table for every query, best first, in nq x k memory: between bbh_jt_assign (k = 1 gives its
 * three outputs) and bbh_jt_dist_matrix (the stable argsort of whose row q, cut at k, is out_idx[q * k .. q * k + k)).
 * The order is bbh_jt_assign's: the smaller (u - i) / u with 0 where u == 0, then the smaller index; it is decided on the
 * exact integers at every row width, never on rounded quotients.  1 <= nc < 2^31; query rows q_stride bytes apart.
 * exclude: optional, nq int32; query q skips row exclude[q] (a value outside [0, nc) skips nothing): a table against
 * itself without the trivial match.  Needs 1 <= k <= BBH_TOPK_MAX and k <= nc (k <= nc - 1 when exclude is given).
 * out_idx: nq x k int32, row-major; out_inter / out_union: optional nq x k uint32, the pairs' exact counts (true union, 0
 * allowed).  The result does not depend on the kernel that served the call or on how the grid was split. */
#define BBH_TOPK_MAX 64
int bbh_jt_topk(const uint8_t* queries, int64_t nq, int64_t q_stride, const uint8_t* rows, int64_t nc, int64_t nbytes,
                int32_t k, const int32_t* exclude, int32_t* out_idx, uint32_t* out_inter, uint32_t* out_union, void* stream);

/* Every row of a table within a Jaccard distance of every query, as CSR: the threshold twin of bbh_jt_topk.  A pair
 * (query q, row m) with i = popcount(q & m) and u = |q| + |m| - i is a hit iff d <= radius in float64, where d is
 * bbh_jt_dist_matrix's value: (u - i) / u as one float64 division, 0.0 where u == 0.  Query q's hits are exactly
 * flatnonzero(dist_matrix[q] <= radius), in ascending row index, at every row width: a pair at the radius bit for bit is
 * a hit, one ulp above is not; radius < 0 gives nothing, radius >= 1 every row.  1 <= nc < 2^31; query rows q_stride bytes
 * apart.  exclude: optional, nq int32; query q skips row exclude[q] (a value outside [0, nc) skips nothing).
 * The size of the answer is not known before the call, so the call works like snprintf.  It always writes out_offsets
 * (nq + 1 int64, out_offsets[0] = 0) and *out_total = out_offsets[nq], which may exceed 2^31.  If total <= capacity it also
 * writes the first total entries of out_idx (int32 row numbers) and of the optional out_inter / out_union (uint32 exact
 * counts, true union, 0 allowed), query q's at [out_offsets[q], out_offsets[q + 1]), and nothing beyond them.  If total >
 * capacity it writes none of the three and still returns BBH_OK: the caller compares *out_total with capacity and calls
 * again.  capacity = 0 with null outputs is the pure count.  BBH_ERR_INVALID, with nothing written: a NaN radius, capacity <
 * 0, a null out_offsets or out_total, capacity > 0 with a null out_idx.  Every pointer may be host or device memory.  The
 * call synchronises the stream.  The result does not depend on the kernel that served the call or on how the grid was split. */
int bbh_jt_radius(const uint8_t* queries, int64_t nq, int64_t q_stride, const uint8_t* rows, int64_t nc, int64_t nbytes,
                  double radius, const int32_t* exclude, int64_t capacity, int64_t* out_offsets, int64_t* out_total,
                  int32_t* out_idx, uint32_t* out_inter, uint32_t* out_union, void* stream);

/* The connected components of a table at a Jaccard distance, without storing an edge: what a union-find over the CSR of
 * bbh_jt_radius(rows, rows, radius) would give.  Rows a and b are linked iff that call reports the pair: d <= radius in
 * float64, d = (u - i) / u as one division, 0.0 where u == 0; a pair at the radius bit for bit is linked, one ulp above is
 * not.  Components are the transitive closure: radius < 0 gives n of them, radius >= 1 one, radius = 0 groups identical rows
 * (and the all-zero rows with each other).  rows: n x nbytes, contiguous; 0 <= n < 2^31.
 * out_root: n int32, the smallest row index of the row's component.  out_label: n int32, the rank of that root among the
 * roots in ascending order, 0 .. count - 1 (scipy.sparse.csgraph.connected_components' labelling).  *out_count: the number
 * of components.  Each output is optional, one at least is needed.  n == 0 is BBH_OK and writes *out_count = 0 only.
 * BBH_ERR_INVALID, with nothing written: a NaN radius, n < 0, n >= 2^31, nbytes <= 0, all three outputs null.  Every
 * pointer may be host or device memory.  The call synchronises the stream.  Device memory beside the operands: 4 bytes per
 * row of popcounts, 4 of forest, 4 more where out_root is null or on the host.  The result is a function of the rows and the
 * radius alone: it does not depend on the kernel that served the call, on how the grid was split or on the order in which
 * workgroups ran. */
int bbh_jt_components(const uint8_t* rows, int64_t n, int64_t nbytes, double radius, int32_t* out_root,
                      int32_t* out_label, int64_t* out_count, void* stream);

/* Leader clustering (sphere exclusion, Taylor-Butina) of a table at a Jaccard distance, without storing an edge.  Rows
 * a != b are neighbours iff bbh_jt_radius(rows, rows, radius) reports the pair: d <= radius in float64, d = (u - i) / u as
 * one division, 0.0 where u == 0; a pair at the radius bit for bit is a neighbour pair, one ulp above is not.
 * density[a] = w[a] + the sum of w[b] over a's neighbours, exact in uint64; w is 1 everywhere where weights is null.
 * Priority: the higher density first; among equal densities the lower row index first, with BBH_LEADERS_TIES_HIGH the higher
 * row index.  The result is what this sequential procedure gives: walk the rows in priority order; a row not yet taken
 * becomes a centre and takes all of its neighbours that are not yet taken; a row already taken is skipped; densities are
 * never recomputed.  Equivalently: the centres are the lexicographically first maximal independent set of the neighbour
 * graph under the priority order (a row is a centre iff none of its higher-priority neighbours is one) and every other
 * row belongs to its highest-priority neighbouring centre.  So every member is within radius of its centre and no two
 * centres are within radius of each other.  radius < 0: every row is its own centre, density = w.  radius >= 1: one
 * cluster around the first row in priority order.  -0.0 is 0: identical rows group, and the all-zero rows with each other.
 * rows: n x nbytes, contiguous, any alignment; 0 <= n < 2^31.  weights: optional, n uint32, 0 allowed.
 * out_centre: n int32, the row index of the row's centre (a centre names itself).  out_label: n int32, the rank of that
 * centre among the centres in ascending row index, 0 .. count - 1 (bbh_jt_components' rule).  *out_count: the number of
 * clusters.  out_density: n uint64.  Each output is optional, one at least is needed.  n == 0 is BBH_OK and writes
 * *out_count = 0 only.  BBH_ERR_INVALID, with nothing written: a NaN radius, n < 0, n >= 2^31, nbytes <= 0, null rows with
 * n > 0, all four outputs null, a flag bit other than bit 0.  Every pointer may be host or device memory.  The call
 * synchronises the stream.  Device memory beside the operands: per row 4 bytes of popcounts and 4 of marks (later the
 * ranks), 8 of densities where out_density is null or on the host, 4 of centres where out_centre is null or on the host;
 * per row that has a neighbour 32 bytes of index maps, state and lists and a copy of the row, rows of up to 256 bytes
 * zero-padded to 8, 16, 32, 64, 128 or 256 bytes.  Host memory: 12 bytes per row while the rows are ranked.  The result is
 * a function of rows, radius, weights and flags alone: it does not depend on the kernel that served the width, on how the
 * grid was split, on the order in which workgroups ran or on BBHIP_LEADERS_ROUNDS (after how many rounds the sequential
 * tail starts). */
#define BBH_LEADERS_TIES_HIGH 1u
int bbh_jt_leaders(const uint8_t* rows, int64_t n, int64_t nbytes, double radius, const uint32_t* weights, uint32_t flags,
                   int32_t* out_centre, int32_t* out_label, int64_t* out_count, uint64_t* out_density, void* stream);

/* Test hook: one v_mfma_i32_16x16x64_i8 with the operand lane maps bb_assign.hip documents.
 * a: 16 x 64 int8, b: 64 x 16 int8, d: 16 x 16 int32 = a @ b, all row-major, host or device. */
int bbh_mfma_i8_probe(const int8_t* a, const int8_t* b, int32_t* d, void* stream);

/* unpack_fingerprints (similarity.cpp:145-214): packed n x nbytes -> n x n_features
 * uint8 of 0/1.  n_features must be a multiple of 8 (same restriction, :163-165). */
int bbh_unpack(const uint8_t* packed, int64_t n, int64_t nbytes, int64_t n_features,
               uint8_t* out, void* stream);

/* pack_fingerprints (fingerprints.py:46-49 = np.packbits(axis=-1), MSB first): n x n_features uint8
 * of 0/non-0 -> n x ceil(n_features/8) packed uint8, the last byte zero-padded. */
int bbh_pack(const uint8_t* unpacked, int64_t n, int64_t n_features, uint8_t* out, void* stream);

/* add_rows (similarity.cpp:381-400): column sums of an n x n_features uint8 array,
 * or, with packed != 0, of the unpacked view of an n x nbytes packed array
 * (jt_isim_packed_u8's inner step, :407-411).  out: n_features uint64. */
int bbh_add_rows(const uint8_t* arr, int64_t n, int64_t n_cols, int packed,
                 int64_t n_features, uint64_t* out, void* stream);

/* centroid_from_sum<uint64_t> (similarity.cpp:216-271; NumPy twin used by the tree,
 * _py_similarity.py:12-42): n_samples <= 1 -> cast; else bit = (2*ls >= n_samples).
 * ls_width: element size of linear_sum in bytes (1, 2, 4 or 8).
 * out: n_features bytes (pack == 0) or ceil(n_features/8) bytes, MSB first. */
int bbh_centroid_from_sum(const void* linear_sum, int32_t ls_width, int64_t n_features,
                          int64_t n_samples, int pack, uint8_t* out, void* stream);

/* jt_isim_from_sum (similarity.cpp:273-301).  *out = NaN and *warn = 1 when
 * n_objects < 2 (the reference raises RuntimeWarning, :275-279).  out is a HOST double. */
int bbh_isim_from_sum(const void* linear_sum, int32_t ls_width, int64_t n_features,
                      int64_t n_objects, double* out, int* warn, void* stream);

/* jt_isim_unpacked_u8 / jt_isim_packed_u8 (similarity.cpp:402-411): add_rows then
 * jt_isim_from_sum with n_objects = n. */
int bbh_isim_rows(const uint8_t* arr, int64_t n, int64_t n_cols, int packed,
                  int64_t n_features, double* out, int* warn, void* stream);

/* jt_compl_isim / jt_isim_medoid (_py_similarity.py:65-117) for k independent sets of packed rows in one call.
 * Set g is rows[offsets[g] .. offsets[g+1]) when members == NULL, else rows[members[i]] for i in that range
 * (offsets: k + 1 non-decreasing int64, offsets[0] == 0; members: offsets[k] int64 in [0, n_rows)).
 * out_compl: optional, offsets[k] float64 in set order; out_medoid: optional, k int64 = position INSIDE the set of
 * the FIRST minimum of its complementary iSIMs.  Sets of 1 or 2 rows: NaN / position 0; an empty set is
 * BBH_ERR_INVALID, and so are an entry of members that is not a row and a set with n_features * m * m >= 2^63
 * (the exact uint64 moments would not fit).  n_features % 8 == 0, n_features <= nbytes * 8.  All pointers host or
 * device.  Recorded by bbh_profile_* as "compl_isim_seg/small" (sets a single wave takes) and
 * "compl_isim_seg/large", "compl_isim_seg" is their sum; units = rows. */
int bbh_compl_isim_segments(const uint8_t* rows, int64_t n_rows, int64_t nbytes, int64_t row_stride,
                            const int64_t* members, const int64_t* offsets, int64_t k, int64_t n_features,
                            double* out_compl, int64_t* out_medoid, void* stream);

/* What the clustering indices of bblean/metrics.py need of every cluster, for k sets of packed rows in one call.  Sets,
 * members, offsets, n_features, residency and every refusal are those of bbh_compl_isim_segments; a refused call writes
 * nothing.  centrals: optional k x n_features/8 bytes, centrals_stride bytes apart (>= n_features/8; 0 when centrals
 * is NULL, anything else is BBH_ERR_INVALID).  Every output is optional:
 *   out_centroids  k x n_features/8 uint8   majority-vote centroid of each set = centroid_from_sum(column sums, m,
 *                                           pack=True): a bit is set where 2 * count >= m; for m == 1 the row itself
 *   out_isim       k float64                jt_isim_from_sum(column sums, m) from the exact uint64 moments; NaN for m < 2
 *   out_dist       offsets[k] float64       set order: 1.0 - inter / max(double(union), 1.0) of every member against its
 *                                           set's central, centrals[g] when given, else the set's centroid
 *                                           (1 - jt_sim_packed(clust, central), metrics.py:100 and :134)
 *   out_sums       k x n_features uint64    column sums of each set in feature order (MSB-first unpacking)
 * Recorded by bbh_profile_* as "cluster_stats_seg/small" (sets a single wave takes) and "cluster_stats_seg/large",
 * "cluster_stats_seg" is their sum; units = rows. */
int bbh_cluster_stats_segments(const uint8_t* rows, int64_t n_rows, int64_t nbytes, int64_t row_stride,
                               const int64_t* members, const int64_t* offsets, int64_t k, int64_t n_features,
                               const uint8_t* centrals, int64_t centrals_stride, uint8_t* out_centroids,
                               double* out_isim, double* out_dist, uint64_t* out_sums, void* stream);

/* Centrals per tile of the all-pairs kernel behind bbh_dbi_worst_ratios (tests sit at this size and next to it). */
#define BBH_DBI_TILE 64

/* The inner loop of metrics.jt_dbi (bblean/metrics.py:149-158) without a k x k array:
 *   out_worst[i] = max over j != i of (scatter[i] + scatter[j]) / (1.0 - inter_ij / max(double(union_ij), 1.0)),
 * starting from 0.0, in IEEE double operations in that order.  A NaN candidate (0 / 0: identical centrals, no scatter)
 * is skipped as Python's max(max_d, x) skips it, +inf wins; k == 1 gives 0.0.  scatter: k float64, each finite and
 * >= +0.0.  centrals: k rows of nbytes, stride bytes apart.  out_flags: optional, 2 uint32: [0] the ordered pairs
 * (i, j != i) with a denominator of 0 under a non-zero numerator, [1] those where both were 0 (the reference raises a
 * NumPy RuntimeWarning at each).  All pointers host or device.  Recorded as "dbi_pairs"; units = ordered pairs. */
int bbh_dbi_worst_ratios(const uint8_t* centrals, int64_t k, int64_t nbytes, int64_t stride, const double* scatter,
                         double* out_worst, uint32_t* out_flags, void* stream);

/* The pair loop of metrics.jt_isim_dunn (bblean/metrics.py:186-199) in one call: min over all pairs i < j of
 * 1 - jt_isim_from_sum(sums[i] + sums[j], sizes[i] + sizes[j]); 1.0 when there are fewer than two clusters.
 * sums: k x n_features uint64 column sums (host or device), sizes: k uint64; out: host double. */
int bbh_isim_pair_min_gap(const uint64_t* sums, const uint64_t* sizes, int64_t k, int64_t n_features,
                          double* out, void* stream);

/* jt_most_dissimilar_packed (similarity.cpp:413-471).  idx1/idx2 are HOST int64;
 * sims1/sims2: n float64 (host or device). */
int bbh_most_dissimilar(const uint8_t* Y, int64_t n, int64_t nbytes, int64_t n_features,
                        int64_t* idx1, int64_t* idx2, double* sims1, double* sims2,
                        void* stream);

/* ---------------------------------------------------------------------------------- */
/* Stateful tree engine -- the per-fingerprint loop of BitBirch.fit / _fit_buffers      */
/* (bitbirch.py:769-787, :848-866) with everything it calls: _BFNode.insert_bf_subcluster*/
/* (:305-357), _BFSubcluster.merge_subcluster/update (:488-526), the merge criteria      */
/* (_merges.py), centroid_from_sum (_py_similarity.py:12) and _split_node (:162-211).    */
/* The whole tree (cluster features, centroids, node tables, leaf chain) is resident in  */
/* HBM; one call inserts a whole batch with the reference's sequential semantics.        */
/* ---------------------------------------------------------------------------------- */

typedef struct bbh_tree bbh_tree;

/* BitBirch.__init__ (bitbirch.py:596-643).  tol_table[old_n] is the adaptive tolerance
 * of _merges.py:113 evaluated by the caller (entries >= tol_len are 0); may be NULL.
 * branching_factor in [2, 1023], n_features a multiple of 8 in [8, 8192]: every corner of that
 * range runs (bf 2 and 1023 at 8 and 8192 features are tested).  *out is NULL after an error. */
int bbh_tree_create(bbh_tree** out, int32_t branching_factor, double threshold,
                    int32_t criterion, double tolerance, const double* tol_table,
                    int64_t tol_len, int32_t n_features, int32_t device);
int bbh_tree_destroy(bbh_tree* t);

/* BitBirch.set_merge (bitbirch.py:674-703).  A branching factor change requires an
 * empty (never fitted or reset) tree, which is how the reference's callers use it: on any
 * other tree it is BBH_ERR_STATE; a branching factor outside [2, 1023] or an unknown
 * criterion is BBH_ERR_INVALID.  A call that is refused (BBH_ERR_INVALID, BBH_ERR_STATE) leaves
 * the tree as it was: criterion, tolerance, table and threshold are only applied once nothing is
 * refused, and the new table is on the device before the old one is released.  (A HIP error
 * while the pools of a new branching factor are set up leaves an empty tree to be destroyed.) */
int bbh_tree_set_merge(bbh_tree* t, int32_t criterion, double tolerance,
                       const double* tol_table, int64_t tol_len, double threshold,
                       int32_t branching_factor);

/* BitBirch.reset (bitbirch.py:1078-1090): drops every node and BitFeature. */
int bbh_tree_reset(bbh_tree* t);

/* BitBirch.fit hot loop (bitbirch.py:769-787): insert n packed fingerprints in order.
 * rows: n rows of n_features/8 bytes, row_stride bytes apart (>= n_features/8); the last row
 * needs only nbytes bytes, so a view that ends where its buffer ends is fine.  n == 0 is
 * BBH_OK whatever rows is; NULL rows with n > 0 are BBH_ERR_INVALID.
 * out_leaf[e] = id of the leaf BitFeature that element e was merged into or created
 * (ids are stable until reset); host or device, may be NULL.  Synchronous. */
int bbh_tree_fit_packed(bbh_tree* t, const uint8_t* rows, int64_t n, int64_t row_stride,
                        uint32_t* out_leaf, void* stream);

/* The same for several independent trees (the shards of multiround's first round,
 * multiround.py:401-422) in ONE kernel launch, one workgroup per tree: the trees insert
 * concurrently on different compute units.  All trees must live on one device.
 * rows[i]: as for bbh_tree_fit_packed - the last row needs only nbytes bytes; rows[i] may be
 * NULL where n[i] == 0 and NULL rows with n[i] > 0 are BBH_ERR_INVALID.  out_leaf, or any
 * out_leaf[i], may be NULL.  Every argument of every tree is checked before the first tree is
 * touched: a NULL entry of trees[] is BBH_ERR_INVALID and no tree has changed. */
int bbh_trees_fit_packed(bbh_tree** trees, int32_t n_trees, const uint8_t* const* rows,
                         const int64_t* n, const int64_t* row_stride, uint32_t* const* out_leaf,
                         void* stream);

/* Route n packed fingerprints through the tree as it stands WITHOUT inserting them: for each
 * row, independently, what _BFNode.insert_bf_subcluster (bitbirch.py:305-357) does up to its
 * first write.  From the root, the first argmax of i / max(u, 1) over the node's rows
 * (i = popcount(row & q), u = |row| + |q| - i; exact fractions, ties to the lower row) is
 * followed down to a leaf row.  rows, row_stride, the last-row rule, n == 0 and NULL rows as
 * for bbh_tree_fit_packed.  Every output is optional (NULL) and may be host or device memory:
 *   out_leaf[e]    id of the chosen leaf BitFeature (the ids bbh_tree_fit_packed writes and
 *                  bbh_tree_export_leaves lists);
 *   out_accept[e]  1 if the tree's current merge criterion (threshold, tolerance, table) would
 *                  accept the row as a one-fingerprint nominee of that BitFeature, else 0
 *                  (BBH_CRIT_NEVER: 0; n_samples + 1 beyond 32 bits: 0);
 *   out_inter[e], out_union[e]  exact counts of the row against that BitFeature's centroid
 *                  (the true union: 0 when both are empty).
 * So inserting row e alone into a copy of the tree merges iff out_accept[e] == 1, and then
 * into out_leaf[e].  The tree is only read: no node is thawed, no pool grows, the counters of
 * bbh_tree_stats / _kernel_counts / _memory and the bytes of bbh_tree_save_fd stay as they were.
 * A tree that holds nothing (never fitted, or reset) is BBH_ERR_STATE (after the n == 0 and
 * NULL checks); a refused call writes nothing.  A walk that would leave the tree (deeper than
 * its recorded depth, a link beyond the pools) ends the call with BBH_ERR_CAPACITY.
 * Synchronous.  Profiled as "tree_route", units = rows. */
int bbh_tree_route_packed(bbh_tree* t, const uint8_t* rows, int64_t n, int64_t row_stride,
                          uint32_t* out_leaf, uint8_t* out_accept, uint32_t* out_inter,
                          uint32_t* out_union, void* stream);

/* _fit_buffers for several independent trees in one launch (the trees of a merge round,
 * multiround.py:240-264): tree i inserts k[i] buffers of element width width[i] from bufs[i].
 * NULL bufs[i] with k[i] > 0 are BBH_ERR_INVALID; checked before the first tree is touched. */
int bbh_trees_fit_buffers(bbh_tree** trees, int32_t n_trees, const void* const* bufs,
                          const int32_t* width, const int64_t* k, uint32_t* const* out_leaf,
                          void* stream);

/* BitBirch._fit_buffers hot loop (bitbirch.py:848-866): insert k BitFeature buffers
 * [linear_sum(n_features) | n_samples], elements of `width` bytes (1,2,4,8), row-major
 * with (n_features+1) columns.  Synchronous.  NULL bufs with k > 0 are BBH_ERR_INVALID.
 * n_samples >= 2^32 (a width-8 table, or a merge that would reach it) is BBH_ERR_INVALID; the
 * tree must be reset (bbh_tree_reset) before it is used again. */
int bbh_tree_fit_buffers(bbh_tree* t, const void* bufs, int32_t width, int64_t k,
                         uint32_t* out_leaf, void* stream);

/* Number of leaf BitFeatures (len(BitBirch._get_leaf_bfs()), bitbirch.py:1216-1222). */
int bbh_tree_leaf_count(bbh_tree* t, int64_t* out);

/* Leaves in leaf-chain order (bitbirch.py:886-893 flattened).  Every output optional
 * (NULL); host or device.  leaf_ids: k uint32; n_samples: k uint64;
 * packed_centroids: k x ceil(F/8) uint8; linear_sums: k x F elements of ls_width bytes
 * (1,2,4,8 -- values must fit; the Python shim asks per dtype group.  A value that does not
 * fit is cast, i.e. its low bits are written). */
int bbh_tree_export_leaves(bbh_tree* t, uint32_t* leaf_ids, uint64_t* n_samples,
                           uint8_t* packed_centroids, void* linear_sums, int32_t ls_width);

/* Gather selected leaves (by position in chain order) as BitFeature buffer rows
 * [linear_sum | n_samples] of `width` bytes -- the table BitBirch._bf_to_np /
 * multiround's round files hold (bitbirch.py:1292-1308, multiround.py:132-143).
 * positions: m int64 (host), any order, repeats allowed; out: m x (F+1) elements, host or
 * device.  A position outside [0, leaf count) is BBH_ERR_INVALID and nothing is written. */
int bbh_tree_gather_buffers(bbh_tree* t, const int64_t* positions, int64_t m,
                            int32_t width, void* out);

/* Packed centroids (np.packbits order, ceil(F/8) bytes each) of the leaves at `positions`
 * (chain order; host int64): BitBirch.get_centroids on a selection (bitbirch.py:895-907).
 * For a leaf BitFeature of one fingerprint this IS its buffer row in packed form, which is
 * how multiround keeps the singleton tail of a uint8 round table (multiround.py:132-143:
 * 2049 bytes per row there) at 256 bytes per row in HBM.  out: m x ceil(F/8), host or device. */
int bbh_tree_gather_centroids(bbh_tree* t, const int64_t* positions, int64_t m, uint8_t* out);

/* counters for tests / profiling: [0] similarity calls, [1] rows compared, [2] merges,
 * [3] appends, [4] splits, [5] nodes, [6] max depth, [7] BitFeature slots used */
int bbh_tree_stats(bbh_tree* t, uint64_t* out8);

/* Which of the three insertion kernels did the work, since the handle was created (tests, bench.py):
 * [0..2] elements inserted by the pipelined / the steady-state / the complete kernel, [3..5] their launches,
 * [6] launches the pipelined kernel ended because the tree had a shape it does not handle, [7] launches that
 * ended because a pool was exhausted (the host grew it and relaunched). */
int bbh_tree_kernel_counts(bbh_tree* t, uint64_t* out8);

/* The level-systolic kernel (one tree over many workgroups: every node has an owner workgroup, elements flow down
 * the levels through one-way rings; the reference's order per node - bitbirch.py:305-357 - by construction; its
 * elements also count as "pipelined" in bbh_tree_kernel_counts): [0] elements it inserted, [1] its launches,
 * [2] relaunches after a root split, [3] workgroups of the last launch, [4] shader cycles its workgroups spent on
 * elements (not waiting), summed, [5] those of workgroup 0 (the root's owner), [6] of the busiest other
 * workgroup (summed over launches), [7] launches it refused (a shape it does not take).
 * Opt-in: BBHIP_SYS=1 uses it wherever the shape allows, =auto where the other kernels are weakest (informative root);
 * unset or 0 (the default): never - its hand-over between workgroups is not dependable yet, DESIGN.md 6s. */
int bbh_tree_sys_counts(bbh_tree* t, uint64_t* out8);

/* What the tree holds in HBM and what its node storage did (tests, tools/config45.py, bench.py):
 * [0] bytes of the node pools (capacity), [1] bytes of their used part, [2] bytes of the uint8 / uint16 / uint32
 * cluster-feature pools (capacity), [3] largest sum of this tree's allocations so far (a pool that is being regrown
 * counts twice), [4] compactions of the node pools, [5] nodes the last one sealed (length rounded up to a block of rows
 * instead of bf + 1 rows: the reference's node is a list that grows, bitbirch.py:264-287), [6] nodes it left at full
 * capacity, [7] sealed nodes moved back to full capacity because an insertion reached them. */
int bbh_tree_memory(bbh_tree* t, uint64_t* out8);

/* Compact the node pools now (the engine does it on its own when pools beyond BBHIP_GC_MIN_MB, default 1024, have to
 * grow): seal != 0 seals every node whose length is what the previous compaction recorded, seal == 0 brings every node
 * back to full capacity.  Results of later calls do not depend on when or whether this ran. */
int bbh_tree_compact(bbh_tree* t, int32_t seal);

/* Tree images: one fitted tree as a self-contained, relocatable byte stream (INTEGRATION.md "Tree files" has the layout;
 * the reference pickles its Python node objects, bitbirch.py:1321-1353).  An image holds every live node at the capacity of
 * a sealed node (the root at full capacity), the used prefixes of the cluster-feature pools, the counters, the statistics
 * of bbh_tree_stats and the configuration (branching factor, n_features, threshold, criterion, tolerance and its table);
 * it holds no pool capacity, no profile or kernel-choice state.
 *
 * bbh_tree_save_fd writes the image at fd's current offset and leaves the tree exactly as it was (no pool is reallocated,
 * no node id changes).  Beyond two uint32 per used block of the node pools (and the scan's few KB) it holds `stage_bytes`
 * of HBM and as much pinned host memory: the image is produced and written in ranges of that size.  stage_bytes == 0
 * means 64 MiB; the smallest value accepted is BBH_TREE_IMAGE_MIN_STAGE(n_features), anything in between is rounded
 * down to a multiple of it.  The bytes written do not depend on stage_bytes.  *written (optional) = bytes of the image.
 *
 * bbh_tree_load_fd reads an image from fd's current offset into a NEW tree on `device` (pools sized as a compaction sizes
 * them: what is live and a quarter more) and leaves the offset behind the image.  The handle is accepted by every other
 * entry point; its nodes are sealed, insertions thaw what they reach, and no result depends on that (bbh_tree_compact).
 * The image is checked as bbh_tree_image_check_fd checks it BEFORE the device sees any of it.
 *
 * bbh_tree_image_check_fd is host code and needs no device: magic, version, byte order, section lengths against the
 * header's counts, truncation; then the structure, from headers, links and row records alone (centroid bytes are never
 * read): every child link and leaf-chain link names a block that starts a live node, lengths <= capacities <= bf + 1,
 * every cluster-feature slot lies below its tier's count (both words of a leaf row that carry one: the row record's and
 * the link word; rows of internal nodes must name the uint32 tier), the leaf chain visits every leaf once and ends,
 * every internal node has a child, every node hangs off the root once and every leaf lies on the recorded depth.  It keeps 32 bytes of host memory per image block while it
 * runs and leaves fd's offset where it was.  Anything wrong: BBH_ERR_INVALID and a message.
 * check and load read with pread: fd must be a regular file.  Profile records: "tree_image/save", "tree_image/load"
 * (the device part of a call; units = image bytes). */
#define BBH_TREE_IMAGE_MIN_STAGE(n_features) \
    ((uint64_t)64 * (4 * ((((uint64_t)(n_features) / 8) + 15) / 16 * 16) + 176))
int bbh_tree_save_fd(bbh_tree* t, int fd, uint64_t stage_bytes, uint64_t* written);
int bbh_tree_load_fd(bbh_tree** out, int fd, int32_t device, uint64_t stage_bytes);
int bbh_tree_image_check_fd(int fd, uint64_t* image_bytes);

/* Per-kernel timing with HIP events on the stream each kernel is launched on.
 * bbh_profile_enable(1) turns it on; bbh_profile_get returns launches and summed
 * milliseconds for the kernel called `name` ("jt_arr_vec", "tree_insert", ...; the tree kernels are recorded as
 * "tree_insert/pipe", "tree_insert/fast" and "tree_insert/complete", "tree_insert" is their sum). */
int bbh_profile_enable(int on);
int bbh_profile_reset(void);
int bbh_profile_get(const char* name, int64_t* launches, double* total_ms);
/* work units (rows / inserted elements) summed over the recorded launches of `name` */
int bbh_profile_units(const char* name, int64_t* units);
/* the longest single recorded launch of `name`: its milliseconds and its work units (the dominant launch of a fit,
 * next to which the short probe / warm-up launches of the same name would only blur an average) */
int bbh_profile_longest(const char* name, double* ms, int64_t* units);

#ifdef __cplusplus
}
#endif
#endif
