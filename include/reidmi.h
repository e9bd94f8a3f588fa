/*
 * reidmi.h — C ABI of libreidmi.so, the MI355X-native CLIP-ReID inference +
 * retrieval path.  Plain pointers and sizes only: every pointer argument is a
 * device pointer (caller-owned, e.g. torch tensor .data_ptr()) unless noted; every
 * call is stream-ordered on `stream` (a hipStream_t passed as void*) and never
 * allocates or synchronises, so a caller may capture it into a hipGraph.
 * Return value: 0 on success, non-zero status with reidmi_last_error() set.
 *
 * The reference (SuperbTUM/Multimodal-ReID) is pure Python with no FFI; each entry
 * point below names the reference function whose semantics it implements.  The
 * Python binding (ctypes) that re-exports the reference call surface lives in
 * multimodal-reid_amd/_lib.py; INTEGRATION.md shows how a reference checkout
 * would bind it.
 */
#ifndef REIDMI_H
#define REIDMI_H
#include <stdint.h>

#include "reidmi_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REIDMI_OK 0
#define REIDMI_EINVAL 1
#define REIDMI_EHIP 2
#define REIDMI_ECAP 3

const char* reidmi_last_error(void);
/* 4 since round 4: the A/B-only entry points (forced GEMM tiling, distance-kernel variant, the
 * fused QKV + attention kernel) moved to the tools library (include/reidmi_tools.h).
 * 5: reidmi_rr_jaccard_topk_rows / reidmi_rr_jaccard_topk_workspace_bytes added.
 * 6: reidmi_search_merge_f32 added.
 * 7: reidmi_combine_rows_f32 added.
 * 8: reidmi_eval_feat_f32 and the reidmi_evf_* stages added.
 * 9: reidmi_search_bounded_f32 added.
 * 10: reidmi_dbscan_f32 added.
 * 11: reidmi_rr_jaccard_self_rows and reidmi_dbscan_jaccard added.
 * 12: reidmi_pair_stats_f32 added.
 * 13: reidmi_search_prefiltered_f32, reidmi_search_prefilter_applies and
 *     reidmi_search_prefiltered_workspace_bytes added.
 * 14: reidmi_search_filter, reidmi_search_filtered_f32 and reidmi_search_prefiltered_filtered_f32
 *     added. */
int reidmi_abi_version(void);

/* ------------------------------------------------------------ retrieval back end */

/* sum_k x[i,k]^2 as an fmaf chain over k ascending (building block of the two below). */
int reidmi_row_sqnorm_f32(const float* x, int64_t n, int64_t d, int64_t ldx, float* out, void* stream);

/* torch.nn.functional.normalize(feats, dim=1, p=2)  — evaluate.py:114.
 * ws: n floats. */
int reidmi_l2norm_f32(const float* x, int64_t n, int64_t d, int64_t ldx, float* y, int64_t ldy, float* ws,
                      void* stream);

/* euclidean_distance(qf, gf) — evaluate.py:7-13 (also reranking.py:36-41 with q = g = feat).
 * out[i*ldo+j] = (||q_i||^2 + ||g_j||^2) - 2 q_i.g_j in exact fp32 (v_mfma_f32_32x32x2_f32).
 * ws: Q+G floats. */
int reidmi_distmat_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                       float* out, int64_t ldo, float* ws, void* stream);

/* Reduced-precision mode of euclidean_distance (SURVEY.md §8b "reidmi_distmat ... mode"):
 * out[i*ldo+j] = (||q_i||^2 + ||g_j||^2) - 2 fp16(q_i).fp16(g_j), the dot products on the fp16
 * MFMA GEMM (fp32 accumulation), the squared norms exact fp32.  Not bit-exact with the
 * reference (reidmi_distmat_f32 is); |error| <= 2^-8 ||q_i|| ||g_j|| per entry (fp16-range rows).
 * The GEMM's epilogue writes the distances straight into out (no product buffer).
 * ws: reidmi_distmat_f16_workspace_bytes(Q, G, D) bytes (fp16 copies padded to the GEMM tile,
 * the squared norms). */
int64_t reidmi_distmat_f16_workspace_bytes(int64_t Q, int64_t G, int64_t D);
int reidmi_distmat_f16(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                       float* out, int64_t ldo, void* ws, int64_t ws_bytes, void* stream);

/* cosine_similarity(qf, gf) — evaluate.py:16-26: arccos(clip(q.g / (|q||g|), -1+1e-5, 1-1e-5)).
 * Same tiling as reidmi_distmat_f32; ws: Q+G floats. */
int reidmi_cosine_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                      float* out, int64_t ldo, float* ws, void* stream);

/* np.argsort(x, axis=1)[:, :k] with ties in index order (kind="stable") — evaluate.py:40,
 * reranking.py:48.  row_div (nullable): rows are divided by row_div[row] first
 * (reranking.py:46 column-max normalisation of a symmetric distance).  Any k <= cols (k > 1024
 * runs in rounds of 1024, one stream over the row each).
 * out_val (nullable) receives the selected values. */
int reidmi_topk_rows_f32(const float* x, int64_t rows, int64_t cols, int64_t ldx, const float* row_div, int k,
                         int32_t* out_idx, float* out_val, int64_t ldo, void* stream);

/* Ranked retrieval: the k nearest gallery rows of every query row, without a Q x G matrix.
 * out_idx[i*ldo + 0..k) / out_dist[i*ldo + 0..k) (out_dist nullable) are, bit for bit, what
 * reidmi_distmat_f32 followed by reidmi_topk_rows_f32(k, row_div = NULL) gives on the same
 * inputs: the same fp32 distances, ascending, ties by gallery index.  The selection runs in the
 * distance kernel's epilogue; the gallery is cut into ranges (a pure function of Q, G, k) whose
 * partial lists a small kernel merges.
 * Labels: all four arrays or none.  With labels, gallery item j is skipped for query i when
 * g_pids[j] == q_pids[i] && g_cams[j] == q_cams[i] (evaluate.py:46-48), and a row with fewer
 * than k items left is padded with index -1 and distance +inf.
 * 1 <= k <= min(G, 128); a larger k is refused (reidmi_distmat_f32 + reidmi_topk_rows_f32 is
 * the route).  Features must be finite.  Any D, ldq, ldg and alignment reidmi_distmat_f32
 * accepts (rows that are not 16-byte aligned, or D % 4 != 0, run the single-stage mainloop).
 * ws: reidmi_search_workspace_bytes(Q, G, D, k) bytes, 16-byte aligned (the squared norms and
 * the ranges' candidate lists: 8 * 128 * ceil(Q / 128) * ranges * cap bytes, cap = 256 for
 * k <= 64, else 384, at most 1024 lists of 128 rows unless Q > 131072; ws_bytes is checked).
 * No allocation or synchronisation inside. */
int64_t reidmi_search_workspace_bytes(int64_t Q, int64_t G, int64_t D, int k);
int reidmi_search_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                      int k, const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                      const int64_t* g_cams, int32_t* out_idx, float* out_dist, int64_t ldo, void* ws,
                      int64_t ws_bytes, void* stream);

/* reidmi_search_f32 under a per-query bound: only admissible items are ranked, and a row with
 * fewer than k of them is padded with -1 / +inf.  The bound is the initial value of the row's
 * running threshold, so the epilogue filters against it from the first tile on: nothing
 * inadmissible enters a candidate list (a gallery block that cannot improve a carried list costs
 * its distance tiles and nothing else).
 * Bound of query i: bd = bound_dist[i*ldb], bi = bound_idx[i*ldb] (device fp32 / int32; the pitch
 * ldb lets a caller pass column k-1 of a carried [Q][k] list in place).
 * Gallery item j, at the distance d reidmi_distmat_f32 gives, is admissible for query i iff it
 * passes the label predicate and
 *     d < bd,
 *  or d == bd and bound_idx == NULL             (the inclusive radius form: d <= bd),
 *  or d == bd and index_base + j < bi           (the strict key form: (d, index_base + j) before
 *                                                (bd, bi) in the order of the rank lists).
 * index_base places this gallery's item j at index_base + j in the bound's index space (the items
 * searched before this block); out_idx stays local to this gallery, as reidmi_search_f32's, so the
 * rows feed reidmi_search_merge_f32 with base = index_base as before.  bi = 2^31 - 1 admits every
 * tie at bd (the radius form for that row alone); bi <= index_base admits none.
 * Output: the min(k, admissible) smallest admissible items by (d, j), bit for bit what
 * reidmi_distmat_f32 + that filter + a stable top-k give, then the padding.
 * bound_dist = +inf admits every finite distance whatever bound_idx holds (a not-yet-full carried
 * list: +inf / -1); a NaN or -inf bound_dist admits nothing.
 * bound_dist == NULL: bound_idx must be NULL too, and the call is reidmi_search_f32 bit for bit.
 * Refused: bound_idx without bound_dist; ldb < 1; index_base < 0 or index_base + G > 2^31 - 1; and
 * whatever reidmi_search_f32 refuses: shapes, k, labels, alignments and the workspace
 * (reidmi_search_workspace_bytes(Q, G, D, k)) are its own. */
int reidmi_search_bounded_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                              int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                              const int64_t* g_cams, const float* bound_dist, const int32_t* bound_idx, int64_t ldb,
                              int64_t index_base, int32_t* out_idx, float* out_dist, int64_t ldo, void* ws,
                              int64_t ws_bytes, void* stream);

/* reidmi_search_bounded_f32 with an fp16 pre-filter: the same rank lists, bit for bit, for most rows
 * at a fraction of the exact search's fp32 MFMA work.  An fp16 MFMA product bounds every exact
 * distance from above (hi) and, through the row's bound width w, from below (hi - w); a sample of
 * the gallery (every sample_stride-th item) gives each row a threshold T = min(the k-th smallest hi
 * among the sample items the label rule leaves, the row's bound distance); a second fp16 product
 * over the whole gallery keeps, in its epilogue, only the pairs with hi - w <= T (at most 4096 per
 * row); their exact distances (the chain of reidmi_distmat_f32) are computed, the admissibility of
 * reidmi_search_bounded_f32 is applied to the exact key and the k smallest by (d, j) are written.
 * Every argument up to ldo is reidmi_search_bounded_f32's, with its labels, bound (bound_dist ==
 * NULL: the unbounded search), index_base, padding (-1 / +inf), tie order and refusals.
 * need: device int32 [Q], written for every row.  need[i] == 0: out_idx / out_dist row i hold, bit
 * for bit, what reidmi_search_bounded_f32 writes on the same inputs.  need[i] == 1: the row has no
 * output and the caller runs the exact search for it (more than 4096 survivors: distances too
 * concentrated for the bound to separate; a non-finite bound; or, for every row at once, a feature
 * beyond +-2^15 or not finite, which fp16 cannot hold).
 * sample_stride: S >= 2, or 0 for the default (16).  The sample is floor(G / S) items rounded down to
 * whole 256-column tiles.  reidmi_search_prefilter_applies (a pure host function) returns 1 when the
 * call can run: D padded to 64 is >= 128, and the sample spans at least one 256-column tile and at
 * least 4 k items (and the shapes, k and sample_stride are themselves valid); otherwise 0, and
 * reidmi_search_prefiltered_f32 refuses with REIDMI_EINVAL.
 * stats: device int32 [4], nullable, written by the call: the rows marked in need; the largest
 * survivor count of any row (4097: a row marked by its sample bounds); the candidates whose exact
 * distance was computed, summed over the rows (saturating at 2^31 - 1); 1 if the fp16 range check
 * failed (then every row is marked).
 * ws: reidmi_search_prefiltered_workspace_bytes(Q, G, D, k, sample_stride) bytes (negative: bad
 * shapes or the pre-filter does not apply), 16-byte aligned, holding in 256-byte aligned parts:
 * the call's state (range flag, counters, the gallery's largest norm); the squared norms and norms
 * of q and g (4 (Q + G) bytes each); the sample's norms; the column records (16 bytes per gallery
 * row, padded to 256 rows); one pass's tile list; per pass of query rows the sample bounds
 * (4 bytes x sample items per row), the survivor lists (8 x 4096 bytes per row), counters,
 * widths, thresholds and row records; and the fp16 copies of q and g, zero-padded to the GEMM
 * tile (rows to 256, D to 64).  Queries go through in passes of
 * min(round_up(Q, 256), clamp(2^30 / per-row bytes, 256, 65536) rounded down to 256) rows: a pure
 * function of the shapes, and no term grows with Q x G.
 * Features must be finite.  Every refusal happens before any HIP call.  Q = 0 is a no-op.  No
 * allocation or synchronisation inside. */
int reidmi_search_prefilter_applies(int64_t Q, int64_t G, int64_t D, int k, int sample_stride);
int64_t reidmi_search_prefiltered_workspace_bytes(int64_t Q, int64_t G, int64_t D, int k, int sample_stride);
int reidmi_search_prefiltered_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                  int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams,
                                  const int64_t* g_pids, const int64_t* g_cams, const float* bound_dist,
                                  const int32_t* bound_idx, int64_t ldb, int64_t index_base, int32_t* out_idx,
                                  float* out_dist, int64_t ldo, int sample_stride, int32_t* need, int32_t* stats,
                                  void* ws, int64_t ws_bytes, void* stream);

/* Filtered search: which gallery items a query may match at all.  A host struct of DEVICE pointers;
 * a clause whose pointers are all NULL is absent.  Gallery item j is admitted for query i iff every
 * clause that is present holds (and the label rule of the four label arrays, when those are given):
 *   valid        g_valid[j] != 0                                            (uint8 [G])
 *   camera mask  0 <= g_cam[j] < 64 and bit g_cam[j] of q_cam_mask[i] is set
 *                (int64 [G]; int64 [Q] read as 64 bits)
 *   time window  q_time_lo[i] <= g_time[j] <= q_time_hi[i]                  (int64 [G], [Q], [Q])
 *   group        g_group[j] != q_group[i]                                   (int64 [G], [Q])
 * The clauses are joined by "and": their order does not matter.  The struct is reidmi_filter.h's
 * (included above):
 *     const uint8_t* g_valid;
 *     const int64_t* g_cam;   const int64_t* q_cam_mask;
 *     const int64_t* g_time;  const int64_t* q_time_lo;  const int64_t* q_time_hi;
 *     const int64_t* g_group; const int64_t* q_group; */

/* reidmi_search_bounded_f32 over the admitted items only: its arguments, with flt after the four
 * label pointers.  The lists are, bit for bit, the rows of reidmi_distmat_f32 with the non-admitted
 * entries removed, ranked by (distance, gallery index), cut at k and at the bound, padded with
 * -1 / +inf: a query with fewer than k admitted items gets a short row, one with none an all-padded
 * row.  The bound applies to admitted items only (a carried key is an admitted item's).  The clauses
 * are tested in the kernel's epilogue behind the threshold compare (an item with g_valid == 0 is
 * skipped before it), by the function that holds the label rule; nothing is filtered afterwards.
 * flt == NULL, or every pointer in it NULL: reidmi_search_bounded_f32, bit for bit and kernel for
 * kernel.  A half-given clause (g_cam without q_cam_mask, q_time_lo without q_time_hi or g_time,
 * g_group without q_group, or the reverse) is refused with the clause's name in reidmi_last_error.
 * The struct is read during the call; the arrays it points to must stay valid until the stream has
 * run the call.  Workspace and every other rule: reidmi_search_bounded_f32's. */
int reidmi_search_filtered_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                               int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                               const int64_t* g_cams, const reidmi_search_filter* flt, const float* bound_dist,
                               const int32_t* bound_idx, int64_t ldb, int64_t index_base, int32_t* out_idx,
                               float* out_dist, int64_t ldo, void* ws, int64_t ws_bytes, void* stream);

/* reidmi_search_prefiltered_f32 over the admitted items only: its arguments, with flt in the same
 * position, its workspace (reidmi_search_prefiltered_workspace_bytes) and its need / stats.  The
 * sample threshold is the k-th smallest bound among the ADMITTED sample items and a candidate must
 * be admitted, so rows with need[i] == 0 hold reidmi_search_filtered_f32's bits; the caller runs
 * reidmi_search_filtered_f32 with the same filter for the others.  The survivor lists hold admitted
 * and non-admitted pairs alike, so a selective filter (few admitted sample items, a loose
 * threshold) overflows them and marks many rows: correct, but then the exact call alone is faster.
 * flt == NULL or all-NULL: reidmi_search_prefiltered_f32 bit for bit.  Half-given clauses are
 * refused as above. */
int reidmi_search_prefiltered_filtered_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G,
                                           int64_t ldg, int64_t D, int k, const int64_t* q_pids,
                                           const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                                           const reidmi_search_filter* flt, const float* bound_dist,
                                           const int32_t* bound_idx, int64_t ldb, int64_t index_base,
                                           int32_t* out_idx, float* out_dist, int64_t ldo, int sample_stride,
                                           int32_t* need, int32_t* stats, void* ws, int64_t ws_bytes, void* stream);

/* Joins S partial rank lists per query into one: the lists of a gallery searched in blocks, or
 * on several GPUs a shard each.  List s of query i is in_idx[s*list_stride + i*ldi + 0..k_in) with
 * in_dist laid out the same way: the rows reidmi_search_f32 writes over block s (ascending by
 * (distance, index), ended by -1 / +inf padding; an entry is present iff its index >= 0).
 * base: int64 [S], nullable (= all zero); the global index of an entry is base[s] + index and
 * must fit int32.  out_idx[i*ldo + 0..k) / out_dist (nullable) are the k smallest present
 * entries of the S lists, ascending by (distance, global index), padded with -1 / +inf: ties go
 * by the global index, never by the order in which the lists are passed.  As a (query, item)
 * distance does not depend on the block the item was in, merged block results are, bit for bit,
 * reidmi_search_f32 over the concatenated gallery (given k_in >= min(k, the block's rows)).
 * The caller guarantees that no global index occurs twice in a row's lists.
 * 1 <= k <= 128, 1 <= k_in <= 128, S >= 1, S * k_in < 2^31, ldi >= k_in, ldo >= k,
 * list_stride >= Q * ldi when S > 1; no relation between k and S * k_in is required.  The
 * outputs must not overlap the inputs.  Q = 0 is a no-op.  No workspace, allocation or
 * synchronisation. */
int reidmi_search_merge_f32(const int32_t* in_idx, const float* in_dist, int S, int64_t Q, int k_in,
                            int64_t list_stride, int64_t ldi, const int64_t* base, int k, int32_t* out_idx,
                            float* out_dist, int64_t ldo, void* stream);

/* Per-query part of eval_func — evaluate.py:40-80.  For query q: valid[q] (any match kept),
 * first[q] (0-based kept-rank of the first match), ap[q] (float64 AP exactly as numpy sums
 * it), nkept[q] (gallery items left after same-pid-same-cam removal).  No capacity limit
 * on positives or junk items per query.  overflow: one int32, written 0 by the call (kept for
 * ABI compatibility with builds that had a positive-list capacity). */
int reidmi_eval_rows(const float* dist, int64_t Q, int64_t G, int64_t ldd, const int64_t* q_pids,
                     const int64_t* g_pids, const int64_t* q_cams, const int64_t* g_cams, int32_t* valid,
                     int64_t* first, double* ap, int64_t* nkept, int32_t* overflow, void* ws, int64_t ws_bytes,
                     void* stream);
/* Device workspace bytes (16-byte aligned) for reidmi_eval_rows: the gallery labels packed
 * once per call and the scratch of a query with more positives than fit LDS (O(G)). */
int64_t reidmi_eval_rows_workspace_bytes(int64_t G);

/* Matrix-free scoring: reidmi_eval_rows' per-query results from the features, without the Q x G
 * matrix.  On finite features valid / first / ap / nkept are, bit for bit, what reidmi_distmat_f32
 * followed by reidmi_eval_rows gives on the same inputs, for any cut of the gallery into blocks
 * or shards and any order in which they are processed.  A gallery item's key is (distance, global
 * index), the distance reidmi_distmat_f32's; an item of the query's pid and camera is removed
 * (evaluate.py:46-48); a match (the query's pid, another camera) has as kept-rank the number of
 * kept items with a smaller key.  Two more outputs give mINP: last[q] (int64, the kept-rank of
 * the last match, -1 without one) and npos[q] (int32, the number of matches).
 *
 * The state of a scoring run is caller-owned device memory for Q queries and a capacity `cap`,
 * the most matches any query may have (the caller takes it from the labels):
 *   pos       [Q][cap] 8-byte entries {fp32 distance, int32 global gallery index}
 *   pos_cnt   int32 [Q]   matches met so far (it keeps counting past cap: such a query overflowed)
 *   junk_cnt  int32 [Q]   removed items met so far
 *   hist      int32 [Q][cap + 1]   hist[q][b]: kept items with exactly b matches before them
 *   overflow  one int32
 * The caller zeroes pos_cnt, junk_cnt, hist and overflow.  The stages, in this order:
 *
 * reidmi_evf_matches, once per gallery block (Gb rows, the first one global index `base`):
 * appends every query's matches in the block to pos, each with its exact distance (the scalar
 * fmaf chain the distance kernel is bit-equal to) and base + j, and adds the block's removed
 * items to junk_cnt.  A query that would exceed cap sets *overflow = 1 and writes nothing past
 * its row.  O(Q * Gb) label compares and O(matches * D) arithmetic: no second distance pass.
 * reidmi_evf_append: appends the lists of another block set or rank (src, the same Q and cap;
 * after an all-gather) to dst, dst_cnt += src_cnt, with the same overflow rule.
 * reidmi_evf_sort: sorts every list ascending by key.  Keys are unique, so the result does not
 * depend on the order of the appends.  Lists of up to 512 entries sort in LDS, longer ones in place.
 * reidmi_evf_count, once per gallery block, after the sort: the distance tile of
 * reidmi_search_f32 (same accepted D, pitches and alignments, four workgroups per CU); its
 * epilogue drops removed items and everything after the row's last match (one compare against
 * that key in LDS) and adds 1 to hist[i][b] for the rest, b = the number of the row's matches with
 * a smaller key.  Integer atomics, so blocks and ranks may be counted in any order and their hist
 * arrays summed.
 * reidmi_evf_finish: per query, rank_t = (inclusive scan of hist up to t) - 1, nkept = G_total -
 * junk_cnt, AP summed with n = nkept exactly as reidmi_eval_rows sums it.  A query whose pos_cnt
 * exceeds cap gets valid = -1 (first = last = -1, ap = 0) and sets *overflow = 1.  hist is consumed
 * (overwritten with the ranks).  last and npos are nullable.
 *
 * ws of matches / count: reidmi_evf_workspace_bytes(Q, Gb) bytes, 16-byte aligned (the squared
 * norms).  Refused with REIDMI_EINVAL before any HIP call: a null required pointer, Q < 0, Gb / G
 * / D <= 0 (Q = 0 is a no-op), cap < 1, a pitch < D, base < 0 or base + Gb >= 2^31, a short or
 * misaligned workspace, a missing label array (all four are required).  No allocation or
 * synchronisation inside. */
int64_t reidmi_evf_workspace_bytes(int64_t Q, int64_t Gb);
int reidmi_evf_matches(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t Gb, int64_t ldg, int64_t D,
                       const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                       int64_t base, int cap, void* pos, int32_t* pos_cnt, int32_t* junk_cnt, int32_t* overflow,
                       void* ws, int64_t ws_bytes, void* stream);
int reidmi_evf_append(void* dst_pos, int32_t* dst_cnt, const void* src_pos, const int32_t* src_cnt, int64_t Q,
                      int cap, int32_t* overflow, void* stream);
int reidmi_evf_sort(void* pos, const int32_t* pos_cnt, int64_t Q, int cap, void* stream);
int reidmi_evf_count(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t Gb, int64_t ldg, int64_t D,
                     const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                     int64_t base, int cap, const void* pos, const int32_t* pos_cnt, int32_t* hist, void* ws,
                     int64_t ws_bytes, void* stream);
int reidmi_evf_finish(const int32_t* pos_cnt, int32_t* hist, const int32_t* junk_cnt, int64_t Q, int cap,
                      int64_t G_total, int32_t* overflow, int32_t* valid, int64_t* first, int64_t* last,
                      int32_t* npos, double* ap, int64_t* nkept, void* stream);

/* The stages above in one call for a resident gallery: matches, sort, count, finish, the state
 * inside ws (zeroed by the call, as is *overflow).  ws: reidmi_eval_feat_workspace_bytes(Q, G, D,
 * cap) bytes, 16-byte aligned: the squared norms, Q * cap * 8 bytes of lists, Q * (cap + 1) * 4 of
 * histogram and 8 * Q of counts; no Q x G term (negative on bad arguments). */
int64_t reidmi_eval_feat_workspace_bytes(int64_t Q, int64_t G, int64_t D, int cap);
int reidmi_eval_feat_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                         const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                         const int64_t* g_cams, int cap, int32_t* valid, int64_t* first, int64_t* last,
                         int32_t* npos, double* ap, int64_t* nkept, int32_t* overflow, void* ws, int64_t ws_bytes,
                         void* stream);

/* DBSCAN over the rows of x [N][ldx] fp32 (device, unit column stride, any pitch >= D), from the
 * features: no N x N matrix is formed, the workspace is linear in N, and the result is the same
 * on every run.  The distance d(i, j) is reidmi_distmat_f32's of x against itself, bit for bit (the
 * SQUARED Euclidean distance; its bits are symmetric in i and j), and eps is in those units, the
 * scale of reidmi_search_bounded_f32's radius.
 *   neighbours  j is a neighbour of i iff d(i, j) <= eps or j == i (the diagonal counts whatever
 *               its rounding gave); counts[i] = the number of neighbours of i, itself included
 *   core        core[i] = 1 iff counts[i] >= min_samples, else 0
 *   clusters    the connected components of the core points under the neighbour relation, numbered
 *               0, 1, ... in ascending order of each component's lowest core index
 *   border      a non-core point with a core neighbour takes the smallest cluster number among its
 *               core neighbours' clusters
 *   noise       everything else: labels[i] = -1
 * which is what scikit-learn's DBSCAN (metric="precomputed", on the same distances) labels.
 * Outputs (device): labels int32 [N], counts int32 [N], core uint8 [N], n_clusters one int32.
 * Three passes over the 128 x 128 distance tiles (count, union of the core pairs, border), each the
 * N x N x D work of reidmi_distmat_f32 without its stores; the union and border passes skip the
 * tiles without a core column.  ws: reidmi_dbscan_workspace_bytes(N, D) bytes, 16-byte aligned:
 * the squared norms and three int32 arrays of N entries plus N / 2048 block sums (negative on bad
 * arguments).  Refused with REIDMI_EINVAL before any HIP call: a null pointer, N < 1, N >= 2^31,
 * D < 1, ldx < D, eps negative or not finite, min_samples < 1, a short or misaligned workspace.
 * No allocation or synchronisation inside. */
int64_t reidmi_dbscan_workspace_bytes(int64_t N, int64_t D);
int reidmi_dbscan_f32(const float* x, int64_t N, int64_t D, int64_t ldx, float eps, int min_samples,
                      int32_t* labels, int32_t* counts, uint8_t* core, int32_t* n_clusters, void* ws,
                      int64_t ws_bytes, void* stream);

/* Verification and open-set statistics of a labelled split from the features: the histogram of the
 * genuine and of the impostor distances under the caller's edges, and every query's nearest genuine
 * and nearest impostor item.  No Q x G matrix is formed and the workspace is linear in Q.  These
 * are what TAR@FAR, EER, the open-set detection-and-identification rate and the choice of
 * reidmi_search_bounded_f32's radius or reidmi_dbscan_f32's eps are computed from.
 * Distance: d(i, j) is reidmi_distmat_f32's of q against g, bit for bit (the SQUARED Euclidean
 * distance); the same D, pitches and alignments are accepted (rows that are not 16-byte aligned,
 * or D % 4 != 0, run the single-stage mainloop).  Features must be finite.
 * Classes of the pair (i, j):
 *   removed   q_cams / g_cams given and g_pids[j] == q_pids[i] && g_cams[j] == q_cams[i]
 *             (evaluate.py:46-48); and, with self_base >= 0, the pair with i == self_base + j (the
 *             diagonal of a set compared with itself, also when the set arrives in blocks: self_base
 *             is then the number of rows before this block; -1: no such pair).  Counted nowhere.
 *   genuine   g_pids[j] == q_pids[i], not removed
 *   impostor  g_pids[j] != q_pids[i], not removed
 * q_pids and g_pids are required; q_cams and g_cams are both given or both NULL (nothing is removed
 * for its camera then).
 * Histogram: edges is a HOST array of 1 <= n_edges <= 255 finite, non-decreasing fp32 values.  It is
 * checked and read during the call (it may be freed afterwards) and reaches the kernel by value in
 * its arguments: no copy, no synchronisation.  The bin of a pair is b = #{t : edges[t] < d}, which
 * is np.searchsorted(edges, d, side="left"): bins 0 .. n_edges, and hist[0] + ... + hist[t] is the
 * number of pairs with d <= edges[t], the pairs a radius or an eps of edges[t] admits.  The call
 * ADDS the genuine pairs' bins to hist_pos and the impostor pairs' to hist_neg (device uint64
 * [n_edges + 1] each; the caller zeroes them before the first block).  No counter can overflow: a
 * workgroup counts in 32-bit LDS bins, a 128 x 128 tile adds at most 2^14 to one, and the bins are
 * added to the 64-bit global counters (one add per non-empty bin) and cleared at the end of the
 * workgroup's gallery range and after every 2^17 tiles, so none exceeds 2^31; a global counter
 * holds up to 2^64 - 1 and one call adds fewer than 2^62 pairs.
 * Nearest items: near_pos_* of query i is its nearest genuine item, near_neg_* its nearest impostor,
 * in the order of the rank lists: the smaller d by fp32 `<`, ties by the smaller global index
 * index_base + j; -0.0 ties with +0.0 (and is reported as +0.0; the distance never is -0.0).  The
 * arrays are in/out (device fp32 / int32 [Q]; the caller starts them at +inf / -1, which stands for
 * "no item"): the call lowers a row's (dist, idx) only to a smaller key.  Inside, a workgroup keeps
 * one packed 64-bit key (the distance's bits in an order-preserving form, then the index) per row
 * in LDS, the ranges meet in a 64-bit minimum in the workspace, and a per-row kernel merges that
 * into the in/out arrays.
 * Sums of integers and minima of unique keys: hist_* and near_* are the same for any cut of the
 * gallery into blocks or shards, any order of the blocks and any scheduling.
 * Geometry: reidmi_evf_count's (a workgroup per 128-row query band and contiguous gallery range, at
 * most 1024 workgroups unless Q > 131072, four per CU).
 * ws: reidmi_pair_stats_workspace_bytes(Q, G) bytes, 16-byte aligned: the Q + G squared norms and
 * 16 bytes per query (negative on bad shapes).
 * Refused with REIDMI_EINVAL before any HIP call: Q < 0, G < 1, D < 1, Q or G >= 2^31; a pitch < D;
 * n_edges outside [1, 255]; NULL, non-finite or decreasing edges; a missing pid array; one camera
 * array without the other; index_base < 0 or index_base + G > 2^31 - 1; self_base < -1; a NULL
 * output; a NULL, misaligned or short workspace; NULL features.  Q = 0 is a no-op.  No allocation
 * or synchronisation inside. */
int64_t reidmi_pair_stats_workspace_bytes(int64_t Q, int64_t G);
int reidmi_pair_stats_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                          const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                          const float* edges, int n_edges, int64_t index_base, int64_t self_base,
                          uint64_t* hist_pos, uint64_t* hist_neg, float* near_pos_dist, int32_t* near_pos_idx,
                          float* near_neg_dist, int32_t* near_neg_idx, void* ws, int64_t ws_bytes, void* stream);


/* k-reciprocal re-ranking — re_ranking(probFea, galFea, k1, k2, lambda_value) (reranking.py:29-100),
 * bit-exact with the reference's numpy arithmetic given the same distances (stable ties).
 * feat [Q+G][ldf] fp32 = cat(probFea, galFea).  final_dist [Q][ldo] fp32 = re-ranked q x g
 * distances.  one_minus_lambda_h = np.float16(1 - lambda) bits, lambda_f = np.float32(lambda)
 * (numpy's weak-scalar conversions, reranking.py:95).  Any k1 >= 1, k2 >= 1 and any neighbourhood
 * density (no capacity limit, as the reference): the workspace holds V and V_qe at their
 * worst-case row widths (kf (kh1 + 1) and k2 times that, capped at N) and the scratch of the
 * kernels for rows beyond the on-chip ones.  flags: device int32, 0 after a correct run (8 would
 * mean a row beyond the sized scratch: a bug, reported instead of a fault). */
int64_t reidmi_rerank_workspace_bytes(int64_t Q, int64_t G, int k1, int k2, int from_dist, int need_transpose);
int reidmi_rerank(const float* feat, int64_t Q, int64_t G, int64_t D, int64_t ldf, int k1, int k2,
                  uint16_t one_minus_lambda_h, float lambda_f, float* final_dist, int64_t ldo, void* ws,
                  int64_t ws_bytes, int32_t* flags, void* stream);
/* From a given (Q+G) x (Q+G) distance (reranking.py:33-35 only_local / local_distmat paths):
 * original_dist = dist (+ add, nullable); symmetric = 1 promises original_dist == its
 * transpose (then no transpose pass is made). */
int reidmi_rerank_from_dist(const float* dist, const float* add, int64_t Q, int64_t G, int symmetric, int k1,
                            int k2, uint16_t one_minus_lambda_h, float lambda_f, float* final_dist, int64_t ldo,
                            void* ws, int64_t ws_bytes, int32_t* flags, void* stream);

/* Staged re-ranking: R1-R7 of re_ranking (reranking.py:29-100) as row-range stages over
 * caller-allocated, exactly sized buffers, bit-identical to reidmi_rerank.  The N x N distance
 * is never materialised (chunk_rows x N row blocks are), and every stage takes a row range,
 * so ranks can each own [lo, hi) and all-gather R / V / V_qe between stages.
 * feat [N][ldf] fp32 = cat(probFea, galFea); sqn[N] = squared row norms (reidmi_row_sqnorm_f32).
 * K = min(max(k1 + 1, k2), N) columns of initial_rank.  CSR inputs are (off[N+1] int64, col
 * int32, fp16 bits), columns ascending per row.
 * reidmi_rr_caps: ELL widths vcap (V rows: the bound kf (kh1 + 1), capped at N) and qcap (the
 * V_qe rows reidmi_rr_qe_rows assembles on chip), and the workspace bytes of reidmi_rr_v_rows
 * (0 when k1 <= 61: on chip) and of reidmi_rr_qe_deferred. */
int reidmi_rr_caps(int64_t N, int k1, int k2, int64_t* vcap, int64_t* qcap, int64_t* v_ws_bytes,
                   int64_t* qe_ws_bytes);
/* R1+R2 (reranking.py:36-48): rank_out[hi-lo][K] = stable argsort prefix of od rows lo..hi,
 * rowmax_out[hi-lo] = the od divisors (column maxima of the symmetric distance). */
int reidmi_rr_rank_rows(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn, int64_t lo, int64_t hi,
                        int K, int32_t* rank_out, float* rowmax_out, float* chunk, int64_t chunk_rows, void* stream);
/* R3 (reranking.py:51-71): V rows lo..hi (ELL [hi-lo][vcap]) from the full rank[N][K] and
 * rowmax[N]; distance entries recomputed from feat with the distance kernel's arithmetic. */
/* fp16 copy of the features for reidmi_rr_rank_rows_f16: [Np][Dp] zero-padded (Np % 256 == 0,
 * Dp % 64 == 0); *range_ok (device int32, set to 1 by the caller) is cleared when some |x| > 2^15
 * or is not finite, and the pre-filter must then not be used. */
int reidmi_rr_feat16(const float* feat, int64_t N, int64_t D, int64_t ldf, void* feat16, int64_t Np, int64_t Dp,
                     int32_t* range_ok, void* stream);
/* Largest norm and squared norm over the N items (out2[0], out2[1]: device floats), the input
 * nmax2 of reidmi_rr_rank_rows_f16. */
int reidmi_rr_norm_max(const float* sqn, const float* nrm, int64_t N, float* out2, void* stream);
/* reidmi_rr_rank_rows with an fp16 MFMA pre-filter (same rank_out / rowmax_out bits): the fp16
 * product bounds every exact distance (error bound in prefilter.hip, above rank_select1_kernel); only the
 * candidates are recomputed with the exact fp32 chain.  Default form (sample stride 16, for N
 * >= 4096): per-row thresholds from every 16th item, then the selection runs inside the GEMM's
 * epilogue (survivor lists, no N-wide row in HBM; when one call covers all N rows and the lists
 * fit the chunk, only the upper triangle of the symmetric product runs).  Smaller N: the GEMM's
 * epilogue writes the upper bounds (chunk [chunk_rows][Np] fp32) for a streaming selection.
 * Rows whose distances are too concentrated for the bound (or not finite), or whose survivor
 * list overflows, get need[r] = 1 and no output: the caller runs the exact rows for them.
 * nrm = sqrt(sqn); nmax2 = reidmi_rr_norm_max(sqn, nrm); need [hi - lo] int32; chunk:
 * chunk_rows x Np fp32. */
int reidmi_rr_rank_rows_f16(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn, const float* nrm,
                            const float* nmax2, const void* feat16, int64_t Np, int64_t Dp, int64_t lo, int64_t hi,
                            int K, int32_t* rank_out, float* rowmax_out, int32_t* need, float* chunk,
                            int64_t chunk_rows, void* stream);
/* The same with the sample stride chosen: 0 or 1 = the dense form (bounds written to the chunk,
 * streaming selection) at any N; S >= 2 = the selection inside the GEMM's epilogue against
 * per-row thresholds from every S-th item (prefilter.hip "R2 pre-filter with the selection in the
 * GEMM"), when floor(N / S) spans at least one 256-column tile and 4 K items (else the dense
 * form).  Same output bits.  reidmi_rr_rank_rows_f16 uses S = 16 (rerank_rank.hip RR_SAMPLE_STRIDE):
 * 1M-item R2 1.98 s in the triangle form vs 3.9 s dense. */
int reidmi_rr_rank_rows_f16_ex(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn,
                               const float* nrm, const float* nmax2, const void* feat16, int64_t Np, int64_t Dp,
                               int64_t lo, int64_t hi, int K, int32_t* rank_out, float* rowmax_out, int32_t* need,
                               float* chunk, int64_t chunk_rows, int sample_stride, void* stream);
/* Rows that one internal pass of reidmi_rr_rank_rows_f16(_ex) processes with a chunk of
 * chunk_rows x Np floats (the in-epilogue form needs ~0.3 MB per row at N = 1M instead of 4 N
 * bytes): size the calls' row ranges by it.  sample_stride < 0: the default form's.  -1 on bad
 * arguments. */
int64_t reidmi_rr_rank_rows_f16_pass_rows(int64_t N, int64_t Np, int64_t chunk_rows, int K, int sample_stride);
/* R2's triangle form in stages, for sharding it over ranks (reranking.HipStages under a process
 * group): rank r samples its rows (reidmi_rr_tri_sample, records all-gathered), runs tiles
 * [t0, t1) = its contiguous share of the upper-triangle list over ALL rows
 * (reidmi_rr_tri_survivors), sends the partial survivor lists of each other rank's rows to it
 * (reidmi_rr_sv_pack, all-to-all) which appends them (reidmi_rr_sv_merge), and selects its own
 * rows (reidmi_rr_sv_select): the same rank_out / rowmax_out / need bits as the one-call
 * reidmi_rr_rank_rows_f16 for any number of ranks, at the one-GPU triangle's total MFMA work.
 * Buffers (caller-owned, device): meta [Np] x 16 B, wrow [N] fp32, cnt [N] int32 (0 for rows
 * sampled elsewhere), list [N][cap] x 8 B, sqn_s / nrm_s [ns] fp32, tiles [ntiles] int32, hs
 * [sample_rows][ns] fp32 (may overlay list; the sizes: reidmi_rr_tri_plan; cap = 0: the
 * triangle form does not apply for this chunk). */
int reidmi_rr_tri_plan(int64_t N, int64_t Np, int64_t chunk_rows, int K, int64_t* ntiles, int64_t* cap, int64_t* ns,
                       int64_t* sample_rows);
int reidmi_rr_tri_init(const float* sqn, const float* nrm, int64_t N, int64_t Np, int64_t ns, void* meta, float* sqn_s,
                       float* nrm_s, int32_t* tiles, void* stream);
int reidmi_rr_tri_sample(const void* feat16, int64_t Np, int64_t Dp, const float* sqn, const float* nrm,
                         const float* nmax2, int64_t N, int64_t D, int K, const float* sqn_s, const float* nrm_s,
                         int64_t ns, int64_t a, int64_t b, float* hs, int64_t hs_rows, void* meta, float* wrow,
                         int32_t* cnt, int cap, void* stream);
int reidmi_rr_tri_survivors(const void* feat16, int64_t Np, int64_t Dp, const float* sqn, const float* nrm, int64_t N,
                            int64_t D, const void* meta, const int32_t* tiles, int64_t t0, int64_t t1, int32_t* cnt,
                            void* list, int cap, void* stream);
int reidmi_rr_sv_select(const int32_t* cnt, const void* list, int cap, const float* wrow, const float* feat,
                        int64_t ldf, int64_t D, const float* sqn, int64_t row0, int64_t rows, int K, int32_t* rank_out,
                        float* rowmax_out, int32_t* need, void* stream);
int reidmi_rr_sv_pack(const int32_t* cnt, const void* list, int cap, int64_t rows, const int64_t* off, void* out,
                      void* stream);
int reidmi_rr_sv_merge(int32_t* cnt, void* list, int cap, int64_t rows, const int32_t* add_cnt, const int64_t* add_off,
                       const void* add, void* stream);
/* R3 (reranking.py:51-71): V rows lo..hi (ELL [hi-lo][vcap]) from the full rank[N][K] and
 * rowmax[N]; distance entries recomputed from feat with the distance kernel's arithmetic.
 * ws: reidmi_rr_caps' v_ws_bytes (nullable when 0). */
int reidmi_rr_v_rows(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn, const float* rowmax,
                     const int32_t* rank, int K, int64_t lo, int64_t hi, int k1, int32_t* vcol, uint16_t* vval,
                     int32_t* vnnz, void* ws, int64_t ws_bytes, int32_t* flags, void* stream);
/* off[0..rows] = exclusive scan of nnz[0..rows) (off[rows] = total). */
int reidmi_rr_row_offsets(const int32_t* nnz, int64_t rows, int64_t* off, void* stream);
/* ELL rows -> CSR storage at off[]. */
int reidmi_rr_pack(const int32_t* ell_col, const uint16_t* ell_val, const int32_t* nnz, int64_t rows, int64_t cap,
                   const int64_t* off, int32_t* col, uint16_t* val, void* stream);
/* R4 (reranking.py:73-78): V_qe rows lo..hi (ELL [hi-lo][qcap]) from the full V (CSR).  Rows
 * beyond the on-chip assembly (or every row when k2 > 32) get qnnz = 0 and are listed in
 * dlist[0 .. *dcount) (dlist int32 [hi-lo], dcount device int32, both written by the call);
 * reidmi_rr_qe_deferred then computes them: mode 0 -> their entry counts into qnnz[b], mode 1 ->
 * the rows into CSR at qoff[b] (qoff = offsets of rows lo..hi).  ws: reidmi_rr_caps' qe_ws_bytes. */
int reidmi_rr_qe_rows(const int32_t* rank, int K, int k2, int64_t lo, int64_t hi, const int64_t* voff,
                      const int32_t* vcol, const uint16_t* vval, int32_t* qcol, uint16_t* qval, int32_t* qnnz,
                      int32_t* dlist, int32_t* dcount, void* stream);
int reidmi_rr_qe_deferred(const int32_t* rank, int K, int k1, int k2, int64_t lo, int64_t N, const int64_t* voff,
                          const int32_t* vcol, const uint16_t* vval, const int32_t* dlist, int64_t n_def, int mode,
                          const int64_t* qoff, int32_t* qcol, uint16_t* qval, int32_t* qnnz, void* ws,
                          int64_t ws_bytes, int32_t* flags, void* stream);
/* R5 (reranking.py:80-82): inverted index of the full V_qe (CSR, nnz entries) as CSC with
 * rows ascending per column: coff[N+1], irow[nnz], ival[nnz]. */
int64_t reidmi_rr_csc_workspace_bytes(int64_t N, int64_t nnz);
int reidmi_rr_csc(int64_t N, const int64_t* qoff, const int32_t* qcol, const uint16_t* qval, int64_t nnz, int64_t* coff,
                  int32_t* irow, uint16_t* ival, void* ws, int64_t ws_bytes, void* stream);
/* R6+R7 (reranking.py:84-100): final rows for queries qlo..qhi: out[qhi-qlo][ldo] (G columns).
 * chunk: distance scratch of chunk_rows x G floats (chunk_rows <= 65535); bounds: device
 * scratch of reidmi_rr_jaccard_bounds_bytes(N, G) bytes for the per-column chunk bounds of the
 * inverted lists. */
int reidmi_rr_jaccard_rows(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn,
                           const float* rowmax, int64_t Q, int64_t qlo, int64_t qhi, const int64_t* qoff,
                           const int32_t* qcol, const uint16_t* qval, const int64_t* coff, const int32_t* irow,
                           const uint16_t* ival, uint16_t one_minus_lambda_h, float lambda_f, float* out, int64_t ldo,
                           float* chunk, int64_t chunk_rows, void* bounds, int64_t bounds_bytes, void* stream);
int64_t reidmi_rr_jaccard_bounds_bytes(int64_t N, int64_t G);
/* R6+R7 as ranked lists: for queries qlo..qhi, the k smallest entries of the rows that
 * reidmi_rr_jaccard_rows would write, without those rows.  out_idx[(i-qlo)*ldo + 0..k) /
 * out_dist[(i-qlo)*ldo + 0..k) (out_dist nullable) are, bit for bit, what reidmi_rr_jaccard_rows
 * followed by reidmi_topk_rows_f32(k, row_div = NULL) gives on the same inputs: the same final
 * distances (one definition of the per-element blend for both), ascending, ties by gallery index.
 * The selection runs inside the Jaccard kernel, one sorted partial list per (query, 8192-column
 * chunk); a small kernel merges a query's lists, so the result does not depend on the chunking.
 * The inputs are reidmi_rr_jaccard_rows' (chunk: chunk_rows x G floats, 1 <= chunk_rows <= 65535;
 * bounds as there).
 * Labels: all four arrays or none; q_pids / q_cams are indexed by query row 0..Q, g_pids / g_cams
 * by gallery item 0..G.  With labels, gallery item j is skipped for query i when g_pids[j] ==
 * q_pids[i] && g_cams[j] == q_cams[i] (evaluate.py:46-48), and a row with fewer than k items left
 * is padded with index -1 and distance +inf.
 * 1 <= k <= min(G, 128); a larger k is refused (reidmi_rr_jaccard_rows + reidmi_topk_rows_f32 is
 * the route).  Features must be finite.
 * ws: reidmi_rr_jaccard_topk_workspace_bytes(chunk_rows, G, k) = chunk_rows * ceil(G / 8192) * k * 8
 * bytes, 8-byte aligned: the partial lists of one row pass (no Q x G term; ws_bytes is checked;
 * -1 for arguments the call refuses).  No allocation or synchronisation inside; every refusal
 * happens before any HIP call and leaves its message in reidmi_last_error(). */
int64_t reidmi_rr_jaccard_topk_workspace_bytes(int64_t rows_per_pass, int64_t G, int k);
int reidmi_rr_jaccard_topk_rows(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn,
                                const float* rowmax, int64_t Q, int64_t qlo, int64_t qhi, const int64_t* qoff,
                                const int32_t* qcol, const uint16_t* qval, const int64_t* coff, const int32_t* irow,
                                const uint16_t* ival, uint16_t one_minus_lambda_h, float lambda_f, int k,
                                const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                                const int64_t* g_cams, int32_t* out_idx, float* out_dist, int64_t ldo, float* chunk,
                                int64_t chunk_rows, void* bounds, int64_t bounds_bytes, void* ws, int64_t ws_bytes,
                                void* stream);
/* The Jaccard term alone, of the N items against themselves (reranking.py:86-93 for every row i in
 * [0, N) over every column j in [0, N); the number of queries plays no part in V_qe):
 *   tm(i, j) = the sequential fp16 sum, over the nonzero columns c of V_qe[i] in ascending c, of
 *              min(V_qe[i, c], V_qe[j, c])
 *   jd(i, j) = 1 - tm / (2 - tm), every operation rounded to fp16
 * which is the Jaccard half of reidmi_rr_jaccard_rows' blend, from the same walk: the same bits.
 * The bits are symmetric in i and j; a diagonal entry is small but need not be zero, an entry may
 * be slightly negative (tm rounds above 1), and jd(i, j) = 1 exactly where V_qe[i] and V_qe[j]
 * share no column.  This is the Jaccard distance of the reference's re_ranking; other code bases'
 * compute_jaccard_distance variants build V differently and give other values.
 * out [hi-lo][ldo] uint16 (fp16 bits, ldo >= N): rows lo..hi over all N columns, the dense form for
 * small N.  qoff / qcol / qval: V_qe of all N rows (CSR); coff / irow / ival: its inverted index
 * (reidmi_rr_csc); bounds: reidmi_rr_jaccard_bounds_bytes(N, N) bytes, 8-byte aligned.  Refused
 * with REIDMI_EINVAL before any HIP call: a null pointer, N < 1, N >= 2^31, a row range outside
 * 0 <= lo <= hi <= N, ldo < N, short or misaligned bounds. */
int reidmi_rr_jaccard_self_rows(int64_t N, int64_t lo, int64_t hi, const int64_t* qoff, const int32_t* qcol,
                                const uint16_t* qval, const int64_t* coff, const int32_t* irow,
                                const uint16_t* ival, uint16_t* out, int64_t ldo, void* bounds, int64_t bounds_bytes,
                                void* stream);
/* DBSCAN of the N items on that distance, from the sparse rows: no N x N matrix is formed and the
 * result is the same on every run.  The rules and the outputs are reidmi_dbscan_f32's with d
 * replaced by jd: eps is rounded to fp16 (to nearest even) and compared with the fp16 jd, j is a
 * neighbour of i iff jd(i, j) <= eps16 or j == i; counts, core, clusters numbered by lowest core
 * index, border points to the smallest cluster number, noise = -1 as there.  The rounded eps must
 * satisfy 0 <= eps16 < 1: a pair without a shared column has jd = 1 and is never visited, which
 * is what makes the three passes (count, union of the core pairs, border) sparse.  Each pass runs
 * one workgroup per (row, 8192-column chunk) that returns at once when no inverted list of the
 * row's columns has an entry in the chunk.
 * Inputs: V_qe of all N rows and its inverted index, as for reidmi_rr_jaccard_self_rows.
 * ws: reidmi_dbscan_jaccard_workspace_bytes(N) bytes, 16-byte aligned: three int32 arrays of N
 * entries, N / 2048 block sums, and the chunk bounds of the inverted lists, N * (ceil(N / 8192) + 1)
 * * 8 bytes (11 MB at 100 000 rows, about 1 GB at 1M; negative on bad arguments).  Refused with
 * REIDMI_EINVAL before any HIP call: a null pointer, N < 1, N >= 2^31, eps negative, not finite or
 * rounding to >= 1 in fp16, min_samples < 1, a short or misaligned workspace.  No allocation or
 * synchronisation inside. */
int64_t reidmi_dbscan_jaccard_workspace_bytes(int64_t N);
int reidmi_dbscan_jaccard(int64_t N, const int64_t* qoff, const int32_t* qcol, const uint16_t* qval,
                          const int64_t* coff, const int32_t* irow, const uint16_t* ival, float eps, int min_samples,
                          int32_t* labels, int32_t* counts, uint8_t* core, int32_t* n_clusters, void* ws,
                          int64_t ws_bytes, void* stream);
/* Row utilities of the staged driver's exact-row fallback (reranking.HipStages): row maxima
 * skipping NaN (the od divisors, reranking.py:46); ordered compaction idx[0..*count) = positions
 * of the nonzero flags (np.nonzero; count: device int32); out[r] = x[row0 + idx[r]] (fp32 rows). */
int reidmi_rowmax_f32(const float* x, int64_t rows, int64_t cols, int64_t ldx, float* out, void* stream);
int reidmi_nonzero_i32(const int32_t* flags, int64_t n, int32_t* idx, int32_t* count, void* stream);
int reidmi_gather_rows_f32(const float* x, int64_t ldx, int64_t d, int64_t row0, const int32_t* idx, int64_t n,
                           float* out, int64_t ldo, void* stream);

/* Weighted, indexed combination of feature rows, optionally L2-normalised: the device step of
 * query expansion (q' = normalise(q + sum_i w_i g_nn_i)), database augmentation (the same for
 * every gallery row against the gallery) and group pooling (multi-query, tracklets).
 *   out[r] = f( base_w * base[r]  (if base),  { w[t] * src[idx[t]] : t in [offsets[r], offsets[r+1]) } )
 * mode 0 sum, 1 mean, 2 max.  All fp32.  offsets: device int64 [rows + 1], ascending; idx: device
 * int32; w: device fp32 or NULL (= 1).  Entries with idx < 0 are skipped (reidmi_search_f32's short
 * rows end in -1).  Entries with idx >= n_src are skipped and counted in *bad (device int32,
 * nullable; the caller zeroes it, the call adds).  base (nullable): [rows][ld_base].
 * Arithmetic, fixed bit for bit (a plain float32 loop in this order is the exact oracle):
 *   sum / mean: one fp32 accumulator per column, starting at base_w * base[r][c] (rounded), or +0
 *     without a base; for each kept entry in list order acc = acc + (w[t] * src[j][c]), the product
 *     rounded to fp32, then the sum rounded to fp32: never an FMA.  With w == NULL the term is
 *     src[j][c] itself.  mean then divides by (float)(kept entries + (base ? 1 : 0)); a row with
 *     nothing kept and no base is all +0.
 *   max: the elementwise fmaxf over the base row (if any) and the kept rows; w must be NULL and
 *     base_w is ignored; a row with nothing kept and no base is +0.
 *   normalize != 0: the row is then normalised with reidmi_l2norm_f32's arithmetic (one device
 *     definition, csrc/rownorm.h: the squared norm as one fmaf chain over the columns ascending,
 *     each value divided by max(sqrt(ss), 1e-12)); the result equals reidmi_l2norm_f32 of the
 *     normalize == 0 output bit for bit.
 * Refused before any launch (REIDMI_EINVAL): a null src, offsets, idx or out when rows > 0;
 * d <= 0, ld_src < d, ldo < d, ld_base < d with a base; mode outside 0..2; max given weights;
 * n_src or rows >= 2^31.  rows == 0 is a no-op.  Any d, pitches and alignment (16-byte accesses
 * when all pointers are 16-byte aligned and d and the pitches are multiples of 4).  out must not
 * overlap src or base.  No workspace, allocation or synchronisation. */
int reidmi_combine_rows_f32(const float* src, int64_t n_src, int64_t d, int64_t ld_src,
                            const int64_t* offsets, const int32_t* idx, const float* w, int64_t rows,
                            const float* base, int64_t ld_base, float base_w,
                            int mode, int normalize, float* out, int64_t ldo, int32_t* bad, void* stream);

/* ---------------------------------------------- multi-GPU exchange (RCCL, §8e) */

/* The eval path's one exchange step for callers that are not Python (the Python drop-in uses
 * torch.distributed's "nccl" group, multimodal_reid_amd/distributed.py, with the same layout):
 * gallery feature rows are sharded contiguously over the ranks of one node — rank r of W owns
 * rows [n*r/W, n*(r+1)/W) — embedded locally, all-gathered (reidmi_comm_allgather_rows), each
 * rank scores its own query rows (reidmi_distmat_f32 + reidmi_eval_rows, or the staged re-rank),
 * and the per-query results are all-gathered the same way and reduced on the host in query
 * order (bit-identical CMC/mAP for every W).  RCCL (NCCL API) is opened at first use from
 * librccl.so.1 (torch's copy when torch is loaded).  No collective is made by any other entry
 * point. */
#define REIDMI_COMM_ID_BYTES 128
typedef struct reidmi_comm* reidmi_comm_t;
/* ncclGetUniqueId: rank 0 creates the id (HOST buffer of REIDMI_COMM_ID_BYTES) and hands it to
 * the other ranks out of band (as for ncclCommInitRank). */
int reidmi_comm_unique_id(void* id);
/* One communicator per process; device = the HIP device of this rank. */
int reidmi_comm_init(reidmi_comm_t* comm, int nranks, int rank, const void* id, int device);
int reidmi_comm_destroy(reidmi_comm_t comm);
int reidmi_comm_rank(reidmi_comm_t comm, int* rank, int* nranks);
/* All-gather of contiguous row shards: send = this rank's rows [n*r/W, n*(r+1)/W) of row_bytes
 * each, recv = all n_total rows in order.  scratch: device, reidmi_comm_allgather_rows_scratch_bytes
 * (W * ceil(n_total / W) * row_bytes; the padded in-place all-gather). */
int64_t reidmi_comm_allgather_rows_scratch_bytes(int nranks, int64_t n_total, int64_t row_bytes);
int reidmi_comm_allgather_rows(reidmi_comm_t comm, const void* send, int64_t n_total, int64_t row_bytes, void* recv,
                               void* scratch, int64_t scratch_bytes, void* stream);
/* Sum all-reduce of count elements; dtype 0 = fp32, 1 = fp64, 2 = int32, 3 = int64. */
int reidmi_comm_allreduce(reidmi_comm_t comm, const void* send, void* recv, int64_t count, int dtype, void* stream);

/* ------------------------------------------------------------------ encoders */

/* fp16 GEMM C = A . W^T (+bias) on v_mfma_f32_16x16x32_f16, fp32 accumulation (the
 * reference's GPU dtype: utils.py:145-166 converts Linear/conv/MHA weights to fp16), with an
 * optional folded LayerNorm — the QKV / c_fc GEMMs of the encoders (ln_1 / ln_2 -> in_proj /
 * c_fc, custom_clip_model.py:27-28):
 * out = epi(rstd_m * (A W^T)_mn + (-mean_m rstd_m) * colsum_n + bias_n), rowstat float2
 * (rstd, -mean * rstd) with round_up(M, 256) entries (those past M are read, not used) and
 * colsum [N] fp32, both NULL for a plain GEMM (bias required with them).
 * A [M][lda], W [N][ldw] fp16 (Linear weight layout), N % 128 == 0, K % 64 == 0.
 * epi: 0 -> out fp16 = acc+bias; 1 -> out fp16 = QuickGELU(acc+bias); 5 -> out fp32 = acc+bias;
 *      6 -> out fp16 += acc+bias (sum in fp32, one rounding: the encoders' fp16 residual
 *      stream; no folded LayerNorm: rowstat / colsum NULL).  bias nullable (fp32).  fp16
 *      outputs: ldc % 8 == 0 (< 2^24), 16-byte aligned out. */
int reidmi_gemm_f16(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K,
                    const float* bias, const void* rowstat, const float* colsum, void* out, int64_t ldc, void* stream);

/* The product's timing hook (part of the product ABI on purpose; not an A/B variant — those live
 * in libreidmi_tools.so, reidmi_tools.h).  Measurement hooks: live timing of the GEMM launches (HIP events recorded on the launch stream
 * around each GEMM, including those inside reidmi_vit_forward / reidmi_text_forward), which is
 * how bench.py measures the dominant kernel's average launch time over its timed steps (the
 * roofline `achieved`; no other interface reaches a kernel inside the forward).  Off by
 * default: a disabled hook costs one branch per GEMM launch and records nothing.
 * collect: epi = GEMM epilogue id (-1 = all); returns summed device ms, launch count,
 * algorithmic FLOPs (2MNK) and clears the record. */
int reidmi_prof_enable(int on);
int reidmi_prof_collect(int epi, double* total_ms, int64_t* count, double* flops);
/* Same, counting only launches of >= min_flops (e.g. the full-batch launches of a kernel,
 * so that the average matches that kernel's row in a rocprofv3 --stats summary). */
int reidmi_prof_collect_min(int epi, double min_flops, double* total_ms, int64_t* count, double* flops);

/* Key padding used for an L-token sequence by the attention kernel (rows of v^T). */
int reidmi_attn_lpad(int L);

/* softmax(Q K^T / 8 [+causal]) V per (sequence, head): the SDPA of nn.MultiheadAttention
 * (custom_clip_model.py:22-24; causal text mask maple.py:956-962).  q,k [nseq*H][L][64],
 * vt [nseq*H][64][reidmi_attn_lpad(L)], o [nseq*L][H*64]; all fp16.  L <= 256. */
int reidmi_mhsa_f16(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H, int causal,
                     void* stream);

/* Row length of v^T for an L-token sequence, 1 <= L <= 1024: 32 * ceil(L / 32) + 4, the rule of
 * reidmi_attn_lpad continued past 256 (equal to it up to 256); negative otherwise. */
int reidmi_attn_vt_stride(int L);

/* The same non-causal SDPA for sequences of up to 1024 tokens (the vision tower on square and
 * large crops: 224 x 224 -> 325 tokens, 256 x 256 -> 442, 384 x 384 -> 962).  K and v^T stream
 * through LDS in 64-key tiles with a running row max and sum (online softmax); rounding points
 * as reidmi_mhsa_f16 (fp32 scores, sums and accumulation; P and O rounded to fp16 once).
 * q,k [nseq*H][L][64], vt [nseq*H][64][reidmi_attn_vt_stride(L)], o [nseq*L][H*64]; all fp16,
 * 16-byte aligned.  1 <= L <= 1024.  v^T columns >= L may hold anything (never used); nothing is
 * read behind the last head's K rows or v^T row.  reidmi_vit_forward uses it above 256 tokens
 * and reidmi_mhsa_f16 up to 256. */
int reidmi_mhsa_long_f16(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H,
                         void* stream);

/* LayerNorm over rows of width W in {512,768,1024} (fp32 math, eps) — custom_clip_model.py:43-49.
 * Row r of the output reads input row row_idx ? row_idx[r] : r.  y32 / y16 (fp16) nullable. */
int reidmi_layernorm(const float* x, int64_t rows, int64_t ldx, const int32_t* row_idx, int64_t W,
                     const float* gamma, const float* beta, float eps, float* y32, int64_t ldy32, void* y16,
                     int64_t ldy16, void* stream);

/* The encoder's LayerNorm-fold pieces, exported for tests.  row_stats_f16: st [rows] float2 =
 * (rstd, -mean*rstd) (eps 1e-5) of fp16 rows x [rows][ldx] (W = 512 | 768 | 1024), from a
 * pass over x (pst == NULL) or combined from 64-column partials pst [W/64][rows] float2.
 * gemm_f16_resid_partials: the residual GEMM (epi 6: out = half(out + A W^T + bias)) that
 * also writes those partials of the updated rows, pst[n/64 * M + m] (N % 64 == 0). */
int reidmi_row_stats_f16(const void* x, int64_t rows, int64_t ldx, int64_t W, const void* pst, void* st,
                         void* stream);
int reidmi_gemm_f16_resid_partials(const void* A, int64_t lda, const void* Wt, int64_t ldw, int64_t M, int64_t N,
                                   int64_t K, const float* bias, void* out, int64_t ldc, void* pst, void* stream);

/* Prompt construction — coop.PromptLearner.forward (coop.py:95-110) /
 * maple.VLPromptLearner.construct_prompts (maple.py:57-90): out [B][P+C+S][W] fp32 with
 * out[b] = cat(prefix [P][W], ctx[label[b]] [C][W] of ctx [ncls][C][W], suffix [S][W]).
 * W % 4 == 0.  bad_label (nullable device int32) is set to 1 for a label outside [0, ncls). */
int reidmi_prompt_build(const float* prefix, int P, const float* ctx, int C, const int64_t* label, int64_t ncls,
                        const float* suffix, int S, int64_t B, int W, float* out, int32_t* bad_label, void* stream);

/* Per-block weights of a CLIP transformer block (ResidualAttentionBlock,
 * custom_clip_model.py:8-29 / ResidualAttentionBlock_IVLP, maple.py:579-644).
 * Matrices in PyTorch [out][in] layout, vectors fp32.  ln_1 / ln_2 are folded into the
 * GEMM they feed:
 *   qkv_w = fp16(in_proj_weight * ln_1.weight[None, :]), qkv_b = in_proj_bias + in_proj_weight @ ln_1.bias,
 *   qkv_s[n] = sum_k qkv_w[n][k] (of the fp16 values, summed in double);
 *   fc1_w / fc1_b / fc1_s likewise from mlp.c_fc and ln_2.
 * out_w, fc2_w fp16.  ln1_w ... ln2_b are kept for reference (not read by the kernels).
 * prompt: IVLP VPT_shallow [n_ctx][W] (fp32) that replaces the prompt rows before this
 * block, or NULL. */
typedef struct reidmi_block_weights {
    const float* ln1_w;
    const float* ln1_b;
    const void* qkv_w;
    const float* qkv_b;
    const void* out_w;
    const float* out_b;
    const float* ln2_w;
    const float* ln2_b;
    const void* fc1_w;
    const float* fc1_b;
    const void* fc2_w;
    const float* fc2_b;
    const float* prompt;
    const float* qkv_s;
    const float* fc1_s;
} reidmi_block_weights;

/* Vision tower: custom_clip_model.VisionTransformer (custom_clip_model.py:57-100) and the
 * IVLP variant maple.VisionTransformer (maple.py:722-785) when n_ctx > 0.
 * conv_w: conv1.weight [W][3*P*P] flattened (c,ky,kx) and zero-padded to kpad (multiple of
 * 64), fp16.  proj_t: proj^T [out_dim][W] fp16.  blocks: HOST array of `layers` entries. */
typedef struct reidmi_vit_weights {
    int32_t width, layers, heads, patch, stride, out_dim, grid_h, grid_w, n_ctx, kpad;
    const void* conv_w;
    const float* class_emb;
    const float* pos_emb;
    const float* ln_pre_w;
    const float* ln_pre_b;
    const float* ln_post_w;
    const float* ln_post_b;
    const void* proj_t;
    const float* vpt;
    const reidmi_block_weights* blocks;
} reidmi_vit_weights;

/* Workspace bytes for reidmi_vit_forward at batch B (full = 0: CLS outputs only); -1 for bad
 * weights or more than 1024 tokens (1 + grid_h * grid_w + n_ctx). */
int64_t reidmi_vit_workspace_bytes(const reidmi_vit_weights* w, int64_t B, int full);

/* encode_image: runs resblocks[:11] then resblocks[11] (custom_clip_model.py:91-92, also for
 * deeper towers), ln_post and proj.  images [B][3][H][Wimg] fp32 (images_f16 = 0) or fp16,
 * already normalised; any grid of at most 1024 tokens (1 + grid_h * grid_w + n_ctx: 256 x 128
 * -> 211, 224 x 224 -> 325, 256 x 256 -> 442, 384 x 384 -> 962 at patch 16, stride 12).  tta (nullable, device int32 [B][2]): apply the augmented loader's
 * flip + Pad((10,5)) + crop at (top, left) on the fly (data_prepare.py:263-270).
 * full = 0: out_x12 [B][W] = ln_post(x12)[:,0], out_proj [B][E] = (x12 @ proj)[:,0],
 *           out_x11 [B][W] = x11[:,0] (nullable)          (zero_shot_learning.py:84-87)
 * full = 1: out_x12 [B][L][W], out_proj [B][L][E], out_x11 [B][L][W] (nullable)
 *           — the (x11, x12, xproj) triple of encode_image. */
int reidmi_vit_forward(const reidmi_vit_weights* w, const void* images, int images_f16, int64_t B, int H,
                       int Wimg, const int32_t* tta, int full, float* out_x12, float* out_proj, float* out_x11,
                       void* ws, int64_t ws_bytes, void* stream);

/* Text tower: CLIP.encode_text (maple.py:971-984) from token ids, or
 * text_encoder.TextEncoder.forward (text_encoder.py:14-24) from pre-embedded prompts.
 * tok_emb [vocab][W] fp32, pos_emb [ctx][W] fp32, proj_t = text_projection^T [E][W] fp16. */
typedef struct reidmi_text_weights {
    int32_t width, layers, heads, ctx, vocab, out_dim, n_ctx;
    const float* tok_emb;
    const float* pos_emb;
    const float* ln_final_w;
    const float* ln_final_b;
    const void* proj_t;
    const reidmi_block_weights* blocks;
} reidmi_text_weights;

/* Workspace for N rows at the full ctx (an upper bound for any ctx_used). */
int64_t reidmi_text_workspace_bytes(const reidmi_text_weights* w, int64_t N);

/* tokens: device int64 [N][ctx] (always needed: the EOT row is tokens.argmax(-1)).
 * prompts: device fp32 [N][ctx][W] or NULL (then x = tok_emb[tokens]).  out [N][E] fp32.
 * ctx_used: 0 = all ctx positions; else run on the first ctx_used positions only, which
 * gives the same output when every row's EOT position (argmax) and IVLP prompt rows are
 * < ctx_used (causal mask: rows past the EOT never reach it); n_ctx < ctx_used <= ctx. */
int reidmi_text_forward(const reidmi_text_weights* w, const int64_t* tokens, const float* prompts, int64_t N,
                        int ctx_used, float* out, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------ weight packing (checkpoint boundary, §8b)
 *
 * From the reference's fp32 tensors on the device, in its key layout, to a runnable tower whose
 * device data all lives in one caller-owned buffer (256-byte aligned, reidmi_*_pack_bytes):
 * CLIP-ReID checkpoints hold the vision tower under `image_encoder.*` (utils.py:169-221, loaded
 * into custom_clip_model.VisionTransformer) and the text tower under `text_encoder.*`
 * (zero_shot_learning.py:28-35, loaded into the CLIP text tower); strip the prefix and pass the
 * tensors below.  Packing (the definitions multimodal_reid_amd.model uses, pack.hip): ln_1 / ln_2
 * folded into in_proj / c_fc (W' = fp16(fp32(W gamma)), s = sum of W' rows, b' = fp32(b + W beta)
 * with a compensated fp64 sum), the other matrices cast to fp16 (utils.py:145-166 convert_weights),
 * conv1 flattened and zero-padded to a multiple of 64, proj / text_projection transposed; fp32
 * vectors copied.  Stream-ordered; the sources may be freed once the stream passes the call.
 * out_blocks: HOST array of `layers` entries that out->blocks will point to (keep it alive). */
typedef struct reidmi_block_src {  /* transformer.resblocks.{i}.* */
    const float* ln_1_w;           /* ln_1.weight [W] */
    const float* ln_1_b;           /* ln_1.bias [W] */
    const float* in_proj_w;        /* attn.in_proj_weight [3W][W] */
    const float* in_proj_b;        /* attn.in_proj_bias [3W] */
    const float* out_proj_w;       /* attn.out_proj.weight [W][W] */
    const float* out_proj_b;       /* attn.out_proj.bias [W] */
    const float* ln_2_w;           /* ln_2.weight [W] */
    const float* ln_2_b;           /* ln_2.bias [W] */
    const float* c_fc_w;           /* mlp.c_fc.weight [4W][W] */
    const float* c_fc_b;           /* mlp.c_fc.bias [4W] */
    const float* c_proj_w;         /* mlp.c_proj.weight [W][4W] */
    const float* c_proj_b;         /* mlp.c_proj.bias [W] */
    const float* vpt_shallow;      /* IVLP VPT_shallow [n_ctx][W] (maple.py:617-644), or NULL */
} reidmi_block_src;

/* Vision tower keys (custom_clip_model.py:57-76; maple.py:722-753 for IVLP).  The positional
 * embedding must already be at the (grid_h, grid_w) grid of the stride-12 patches (CLIP-ReID
 * checkpoints are; an OpenAI 224 x 224 grid goes through utils.resize_pos_embed first,
 * utils.py:111-125).  blocks: HOST array of `layers` entries. */
typedef struct reidmi_vit_src {
    int32_t width, layers, patch, stride, out_dim, grid_h, grid_w, n_ctx;
    const float* conv1_w;               /* conv1.weight [W][3][P][P] */
    const float* class_embedding;       /* [W] */
    const float* positional_embedding;  /* [1 + grid_h * grid_w][W] */
    const float* ln_pre_w;
    const float* ln_pre_b;
    const float* ln_post_w;
    const float* ln_post_b;
    const float* proj;                  /* [W][out_dim] */
    const float* vpt;                   /* VPT [n_ctx][W] or NULL */
    const reidmi_block_src* blocks;
} reidmi_vit_src;

/* Text tower keys of CLIP (maple.py:929-984): token_embedding.weight, positional_embedding,
 * transformer.resblocks.*, ln_final.*, text_projection.  blocks: HOST array of `layers`. */
typedef struct reidmi_text_src {
    int32_t width, layers, ctx, vocab, out_dim, n_ctx;
    const float* token_embedding;       /* [vocab][W] */
    const float* positional_embedding;  /* [ctx][W] */
    const float* ln_final_w;
    const float* ln_final_b;
    const float* text_projection;       /* [W][out_dim] */
    const reidmi_block_src* blocks;
} reidmi_text_src;

/* Buffer bytes for the packed tower (-1 on bad shapes). */
int64_t reidmi_vit_pack_bytes(const reidmi_vit_src* src);
int reidmi_vit_weights_pack(const reidmi_vit_src* src, void* buf, int64_t buf_bytes, reidmi_vit_weights* out,
                            reidmi_block_weights* out_blocks, void* stream);
int64_t reidmi_text_pack_bytes(const reidmi_text_src* src);
int reidmi_text_weights_pack(const reidmi_text_src* src, void* buf, int64_t buf_bytes, reidmi_text_weights* out,
                             reidmi_block_weights* out_blocks, void* stream);

/* ------------------------------------------------ ResNet image tower (RN50 / RN101, resnet.hip)
 *
 * custom_clip_model.ModifiedResNet (custom_clip_model.py:186-242), eval mode, the reference's GPU
 * dtype: activations fp16 NHWC in HBM, convolution weights the fp16 cast of the checkpoint's
 * (utils.py:145-166), fp32 accumulation on v_mfma_f32_16x16x32_f16.  BatchNorm is NOT folded into
 * the fp16 weights: it is the fp32 epilogue acc * s_c + t_c with s = gamma / sqrt(var + 1e-5),
 * t = beta - mean * s (fp64 at pack time, stored fp32); then the residual is added in fp32, ReLU
 * applied, and the value rounded to fp16 once. */

/* y = relu?(conv(x, w) * scale + shift (+ resid)): implicit-GEMM convolution, M = B * Ho * Wo
 * output pixels, N = Cout, K = k * k * Cin; per output element one chain over the taps (ky, kx)
 * ascending, then channels ascending; out-of-image taps read as zero.
 * x [B][H][W][Cin], y and resid (nullable) [B][Ho][Wo][Cout] fp16, Ho = (H + 2 pad - k) / stride + 1,
 * pad = k / 2; w [Cout][k][k][Cin] fp16; scale, shift [Cout] fp32; 16-byte aligned.
 * k in {1, 3}, stride in {1, 2}, Cout % 32 == 0, and Cin % 32 == 0 (the MFMA kernel) or Cin == 3
 * with k == 3 and Cout <= 512 (the stem's first convolution: its own small fp32 kernel). */
int reidmi_conv2d_f16(const void* x, int64_t B, int H, int W, int Cin, const void* w, int Cout, int k, int stride,
                      const float* scale, const float* shift, const void* resid, int relu, void* y, void* stream);

/* nn.AvgPool2d(2) on NHWC fp16: y[b][i][j][c] = fp16(((x00 + x01) + x10 + x11) * 0.25) with the
 * sum in fp32 in that order (x00 = x[b][2i][2j][c], x01 its right, x10 / x11 the row below), one
 * rounding.  x [B][H][W][C], y [B][H/2][W/2][C]; H, W even, C % 8 == 0. */
int reidmi_avgpool2_f16(const void* x, int64_t B, int H, int W, int C, void* y, void* stream);

/* One convolution + BatchNorm of the packed tower: w [cout][k][k][cin] fp16, scale / shift fp32. */
typedef struct reidmi_conv_weights {
    const void* w;
    const float* scale;
    const float* shift;
    int32_t cin, cout, k, stride;
} reidmi_conv_weights;

/* Bottleneck (custom_clip_model.py:103-146): conv1 1x1, conv2 3x3, AvgPool2d(stride) when
 * stride > 1, conv3 1x1, + identity (through AvgPool2d(stride) -> down 1x1 -> BN when has_down). */
typedef struct reidmi_bottleneck_weights {
    reidmi_conv_weights conv1, conv2, conv3, down;
    int32_t stride, has_down;
} reidmi_bottleneck_weights;

/* The packed tower.  width = the stem width w (64 for RN50 / RN101); embed = 32 w (the pooled
 * feature width); heads = embed / 64; layers = block counts of layer1..4 (layer2, layer3 stride 2,
 * layer4 stride 1: x4 stays at H/16 x W/16); grid = the attention pool's positional grid
 * (H / 16, W / 16).  pos_emb [1 + grid_h * grid_w][embed] fp32; qkv_w = [q; k; v]_proj.weight
 * [3 embed][embed] fp16, qkv_b [3 embed] fp32; c_w = c_proj.weight [out_dim][embed] fp16, c_b
 * [out_dim] fp32.  blocks: HOST array of layers[0] + .. + layers[3] entries.  tta_pad: the value
 * of a padded pixel of the TTA view per channel, i.e. what a zero pixel becomes under the
 * loader's Normalize, (0 - mean_c) / std_c; the packer sets -1 (Normalize(0.5, 0.5)), a caller
 * with other statistics (ImageNet's, data_prepare.py:268) overwrites it. */
typedef struct reidmi_resnet_weights {
    int32_t width, embed, heads, out_dim, grid_h, grid_w;
    int32_t layers[4];
    reidmi_conv_weights stem[3];
    const float* pos_emb;
    const void* qkv_w;
    const float* qkv_b;
    const void* c_w;
    const float* c_b;
    const reidmi_bottleneck_weights* blocks;
    float tta_pad[3];
} reidmi_resnet_weights;

/* The reference's key layout (fp32 device tensors): conv{i}.weight [Cout][Cin][k][k] with
 * bn{i}.{weight, bias, running_mean, running_var}. */
typedef struct reidmi_convbn_src {
    const float* conv_w;
    const float* bn_w;
    const float* bn_b;
    const float* bn_mean;
    const float* bn_var;
} reidmi_convbn_src;

/* layer{l}.{i}.conv{1..3} / bn{1..3} and downsample.{0,1} (down.conv_w NULL: no downsample). */
typedef struct reidmi_bottleneck_src {
    reidmi_convbn_src conv1, conv2, conv3, down;
} reidmi_bottleneck_src;

/* conv1..3 / bn1..3 (stem), layer1..4, attnpool.{positional_embedding [1 + grid_h * grid_w][32 w]
 * (already at the H/16 x W/16 grid: utils.resize_pos_embed otherwise, utils.py:228-231), q_proj,
 * k_proj, v_proj, c_proj (.weight [out][in], .bias)}.  blocks: HOST array, layer1's first. */
typedef struct reidmi_resnet_src {
    int32_t width, out_dim, grid_h, grid_w;
    int32_t layers[4];
    reidmi_convbn_src stem[3];
    const float* positional_embedding;
    const float* q_w;
    const float* q_b;
    const float* k_w;
    const float* k_b;
    const float* v_w;
    const float* v_b;
    const float* c_w;
    const float* c_b;
    const reidmi_bottleneck_src* blocks;
} reidmi_resnet_src;

/* Packing in the manner of reidmi_vit_weights_pack: one caller-owned 256-byte aligned buffer of
 * reidmi_resnet_pack_bytes (-1 on bad shapes: width % 64 != 0, a block count < 1, out_dim % 128
 * != 0, more than 1024 tokens), stream-ordered; convolution weights re-laid to [Cout][kh][kw][Cin]
 * and cast to fp16, BatchNorm reduced to (s, t) in fp64, the projections cast to fp16.
 * out_blocks: HOST array of sum(layers) entries that out->blocks will point to (keep it alive). */
int64_t reidmi_resnet_pack_bytes(const reidmi_resnet_src* src);
int reidmi_resnet_weights_pack(const reidmi_resnet_src* src, void* buf, int64_t buf_bytes, reidmi_resnet_weights* out,
                               reidmi_bottleneck_weights* out_blocks, void* stream);

/* Workspace bytes of reidmi_resnet_forward for B images of H x Wimg; -1 for bad weights or an
 * unsupported shape (H % 16, Wimg % 16, a grid other than the packed one, > 1024 tokens). */
int64_t reidmi_resnet_workspace_bytes(const reidmi_resnet_weights* w, int64_t B, int H, int Wimg, int full);

/* ModifiedResNet.forward (custom_clip_model.py:227-242) and what inference consumes of it
 * (zero_shot_learning.py:88-90): images [B][3][H][Wimg] fp32 (images_f16 = 0) or fp16, already
 * normalised; tta as for reidmi_vit_forward (flip + Pad((10,5)) + crop at (top, left), pad value
 * w->tta_pad), materialised as an fp16 NHWC view in the workspace before the stem.
 * full = 0: out_pool [B][32 w] = avg_pool2d(x4) over the whole map (fp32 mean of the fp16 x4),
 *           out_proj [B][E] = attnpool(x4)[0].
 * full = 1: the same out_pool, out_proj [L][B][E] (all L = H/16 * Wimg/16 + 1 tokens), and out_x3
 *           [B][16 w][H/16][Wimg/16], out_x4 [B][32 w][H/16][Wimg/16] fp32 NCHW (each nullable).
 * No allocation or synchronisation; ws_bytes >= reidmi_resnet_workspace_bytes is checked. */
int reidmi_resnet_forward(const reidmi_resnet_weights* w, const void* images, int images_f16, int64_t B, int H,
                          int Wimg, const int32_t* tta, int full, float* out_pool, float* out_proj, float* out_x3,
                          float* out_x4, void* ws, int64_t ws_bytes, void* stream);

/* -------------------------------------------------------- inference glue (G1) */

/* zeroshot_classifier (zero_shot_learning.py:42-48): out[c] = normalize(mean over rows
 * [offsets[c], offsets[c+1]) of normalize(feats[row])).  feats [rows][E], offsets device
 * int64 [ncls+1], out [ncls][E]; all fp32. */
int reidmi_class_mean_normalize(const float* feats, const int64_t* offsets, int64_t ncls, int64_t E, float* out,
                                void* stream);

/* zero_shot_learning.py:93,121-126 (non-mm): emb[b] = (cat(x12a,pa) + cat(x12b,pb)) / 2,
 * fp32 [B][W+E] with row stride lde. */
int reidmi_feature_tta_avg(const float* x12a, const float* pa, const float* x12b, const float* pb, int64_t B,
                           int64_t W, int64_t E, float* emb, int64_t lde, void* stream);

/* zero_shot_learning.py:116-122 (mm): emb[b] = cat((x12a+x12b)/2,
 * softmax((1/0.07) * normalize((pa+pb)/2) @ zs^T)), zs [ncls][E] fp32. */
int reidmi_feature_tta_mm(const float* x12a, const float* pa, const float* x12b, const float* pb, const float* zs,
                          int64_t B, int64_t W, int64_t E, int64_t ncls, float* emb, int64_t lde, void* stream);

/* ---------------------------------------------------- test-time transforms (§8f) */

/* transforms.Resize((oh, ow)) -> ToTensor() -> Normalize(mean, std)  — data_prepare.py:257-261
 * (the reference's test transform, applied per image in reidDataset.__getitem__,
 * data_prepare.py:87-92) on a packed batch of decoded RGB images; bit-exact with
 * PIL.Image.resize(BILINEAR) (Pillow 12.2, see oracle/transforms_oracle.c).  JPEG decode
 * stays on the host.
 * pix: device, concatenated HWC uint8 images; meta: device int64 [B][3] = (byte offset of
 * the image in pix, h, w) with 0 < h <= max_h, 0 < w <= max_w (images outside are skipped);
 * mean, stdv: HOST float[3]; out: device [B][3][oh][ow] (ow % 4 == 0), out_dtype 0 = fp32, 1 = fp16 (RNE).
 * The flip / pad / crop of the TTA loader (data_prepare.py:263-270) is applied on these
 * outputs by the encoder (reidmi_vit_forward's tta offsets). */
int reidmi_preprocess_u8(const uint8_t* pix, const int64_t* meta, int64_t B, int max_h, int max_w, int oh, int ow,
                         const float* mean, const float* stdv, int out_dtype, void* out, void* stream);

/* On-chip bytes one workgroup of reidmi_preprocess_u8 needs for sources up to max_h x max_w
 * (the call fails above 160 KiB: resize such images on the host first). */
int reidmi_preprocess_lds_size(int oh, int ow, int max_h, int max_w, int64_t* bytes);

/* ---------------------------------------------------------------- JPEG decode (§8f) */

/* Image.open(path).convert("RGB") — data_prepare.py:87-92 (reidDataset.__getitem__, run in the
 * DataLoader workers of data_prepare.py:275-283) — for a batch of JPEG files, bit-exact with
 * Pillow 12.2 / libjpeg-turbo defaults (islow IDCT, fancy upsampling).  Supported: baseline /
 * extended-sequential Huffman, 8-bit, one scan, grayscale or 3 components at 4:4:4, 4:2:2,
 * 4:2:0.  Two steps:
 *
 * reidmi_jpeg_plan (HOST only, no GPU): parses the headers of files[offsets[i] .. offsets[i+1])
 * (host bytes, offsets int64 [B+1]) and writes
 *   status int32 [B]  0 ok, 1 not a JPEG / truncated, 2 progressive / lossless / arithmetic /
 *                     12-bit / multi-scan, 3 component layout, 4 bad tables;
 *   meta int64 [B][3] (byte offset in the decoded batch, h, w) — the `meta` of
 *                     reidmi_preprocess_u8; zeros for images with status != 0;
 *   info int64 [10]   plan bytes, workspace bytes, decoded bytes, max h, max w, images with
 *                     status != 0, coefficient count, distinct Huffman tables, largest
 *                     per-image plane bytes, B;
 *   plan              when plan != NULL and plan_capacity >= info[0]: a position-independent
 *                     blob the caller copies to the device (call once with plan = NULL to size it).
 *
 * reidmi_jpeg_decode (stream-ordered): files = the same bytes on the DEVICE, plan = the plan on
 * the device, info = the HOST info[10] of the plan call (B must equal info[9]); ws >= info[1]
 * bytes; pix >= info[2] bytes receives the HWC uint8 images; err int32 [B] (device) = the plan
 * status, or 5 where the entropy-coded data does not decode (that image's coefficients are
 * then zero).
 *
 * reidmi_jpeg_plan_ex (HOST only) is reidmi_jpeg_plan with a flags word; flags = 0 is
 * reidmi_jpeg_plan itself.  REIDMI_JPEG_PROGRESSIVE also plans progressive files (SOF2, Huffman,
 * 8-bit, the same component layouts): every scan kind of the format (DC / AC, first /
 * refinement, interleaved or not, restart intervals, tables redefined between scans), bit-exact
 * with Pillow.  The planner then walks such a file to its EOI: status 6 when it ends before
 * (Pillow: "image file is truncated"), 2 when its scans do not deliver every coefficient of
 * every component to full precision (libjpeg smooths such images; that is not reproduced), 1
 * for scan parameters libjpeg rejects.  The plan lists each progressive image's scans, and the
 * high 32 bits of info[5] count those images: reidmi_jpeg_decode (unchanged signature) then
 * runs one more kernel for them and none when there are none.  Sequential files get the same
 * status, meta and pixels with either flags value. */
#define REIDMI_JPEG_PROGRESSIVE 1
int reidmi_jpeg_plan(const uint8_t* files, const int64_t* offsets, int64_t B, void* plan, int64_t plan_capacity,
                     int64_t* meta, int32_t* status, int64_t* info);
int reidmi_jpeg_plan_ex(const uint8_t* files, const int64_t* offsets, int64_t B, int flags, void* plan,
                        int64_t plan_capacity, int64_t* meta, int32_t* status, int64_t* info);
int reidmi_jpeg_decode(const uint8_t* files, const void* plan, const int64_t* info, int64_t B, void* ws,
                       int64_t ws_bytes, uint8_t* pix, int32_t* err, void* stream);

/* ---------------------------------------------------------------- loader file reads (§8f) */

/* The file side of reidDataset.__getitem__ (data_prepare.py:89 `Image.open(path)` in 4
 * DataLoader workers, data_prepare.py:275-283): one batch of encoded files gathered into ONE
 * caller-owned (pinned) host buffer by `nthreads` host threads (<= 0: up to 16), byte ranges
 * split evenly over the threads.  HOST only, no GPU.
 *
 * reidmi_files_size: sizes[i] = byte size of paths[i] (UTF-8 / file-system encoded, NUL-ended),
 *   or -1 where it cannot be opened.
 * reidmi_files_read: dst[offsets[i] .. offsets[i+1]) = the contents of paths[i]; status[i] = 0,
 *   1 (cannot open / read error) or 2 (the size differs from offsets[i+1] - offsets[i]).
 * reidmi_bytes_gather: dst[offsets[i] .. offsets[i+1]) = srcs[i][0 .. offsets[i+1] - offsets[i])
 *   (in-memory files, e.g. Python bytes objects).
 * Each returns an error only for bad arguments; per-file problems go to sizes / status. */
int reidmi_files_size(const char* const* paths, int64_t n, int64_t* sizes, int nthreads);
int reidmi_files_read(const char* const* paths, int64_t n, const int64_t* offsets, uint8_t* dst, int32_t* status,
                      int nthreads);
int reidmi_bytes_gather(const void* const* srcs, int64_t n, const int64_t* offsets, uint8_t* dst, int nthreads);

#ifdef __cplusplus
}
#endif
#endif /* REIDMI_H */
