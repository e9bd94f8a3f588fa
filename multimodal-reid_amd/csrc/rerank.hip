// rerank.hip — k-reciprocal re-ranking (reranking.py:29-100, Zhong et al. CVPR'17) on gfx950.
//
// Stage map, all bit-exact with oracle/reid_oracle.c:
//   R1 distmat over cat(q, g)                    distance.hip distmat (exact fp32)     reranking.py:36-41
//   R2 od = D / colmax, initial_rank[:, :K]      rerank_rank.hip: rowmax + topk (stable ties),      reranking.py:45-48
//                                                or the fp16 pre-filter (prefilter.hip)
//   R3 k-reciprocal expansion + V row            rerank_rows.hip: kreciprocal_kernel  (ELL, fp16)   reranking.py:51-71
//   R4 query expansion V_qe = mean of k2 rows    rerank_rows.hip: qe_kernel           (ELL, fp16)   reranking.py:73-78
//   R5 inverted index                            rerank_rows.hip: csc_count/scan/fill(/sort) (CSC)  reranking.py:80-82
//   R6+R7 Jaccard with sequential fp16 sums, blend with od, slice [:Q, Q:]  rerank_jaccard.hip: jaccard_kernel  reranking.py:84-100
//         ... or, instead of the slice, its first k columns per row in   jaccard_kernel<true> + jaccard_merge_kernel
//         stable argsort order (reidmi_rr_jaccard_topk_rows)
// Two drivers: one-call (reidmi_rerank*, this file: N x N distance materialised, capacity-sized
// ELL rows) and staged (reidmi_rr_*, next to their kernels in the three stage sources: row ranges
// over exactly sized CSR buffers, distance rows in chunks or recomputed, shardable over ranks; see
// multimodal_reid_amd/reranking.py).  What the sources share is rerank.h; the one-call driver
// launches every stage through the launchers declared there, the staged entry points' own.
// The reference keeps V, V_qe as dense N x N fp16 (2 x 35 GB at MSMT17) and loops in Python;
// here V/V_qe are row-sorted ELL (column index + fp16 bits) and the inverted index is CSC,
// so memory is O(N * nnz) and every stage is a data-parallel kernel.
// Arithmetic mirrors numpy exactly: float32 exp = numpy's AVX512F/AVX2 polynomial
// (pinned against numpy 2.2.6), float32 pairwise sum, fp16 ufuncs = op in fp32 then RNE.
#include "backend.h"
#include "rerank.h"

namespace reidmi {

// ---------------------------------------------------------------- workspace
struct RrPlan {
    int64_t dist, tdist, rowmax, rank, vcol, vval, vnnz, qcol, qval, qnnz, cnt, off, cur, irow, ival, dlist, dcount,
        krslab, qeslab, total;
    RrCaps caps;
    KrSlab kr;
    QeSlab qe;
};

// One-call driver: V and V_qe as ELL of their worst-case widths (rr_caps), so no row can
// overflow; the generic kernels' slabs only when a row can need them.
static RrPlan rr_plan(int64_t N, int k1, int k2, bool need_dist, bool need_t) {
    RrPlan p{};
    p.caps = rr_caps(N, k1, k2);
    const RrCaps& c = p.caps;
    const int64_t qw = k2 != 1 ? c.qcap : 0;
    p.kr = kr_slab(c.kf, c.kh1);
    p.qe = qe_slab(c.k2e, c.tcap);
    int64_t o = 0;
    p.dist = o; o = align_up(o + (need_dist ? N * N * 4 : 0) + (need_dist ? N * 4 : 0), 256);
    p.tdist = o; o = align_up(o + (need_t ? N * N * 4 : 0), 256);
    p.rowmax = o; o = align_up(o + N * 4, 256);
    p.rank = o; o = align_up(o + N * (int64_t)c.K * 4, 256);
    p.vcol = o; o = align_up(o + N * c.vcap * 4, 256);
    p.vval = o; o = align_up(o + N * c.vcap * 2, 256);
    p.vnnz = o; o = align_up(o + N * 4, 256);
    p.qcol = o; o = align_up(o + N * qw * 4, 256);
    p.qval = o; o = align_up(o + N * qw * 2, 256);
    p.qnnz = o; o = align_up(o + N * 4, 256);
    p.cnt = o; o = align_up(o + N * 4, 256);
    p.off = o; o = align_up(o + (N + 1) * 8, 256);
    p.cur = o; o = align_up(o + N * 4, 256);
    const int64_t inv = k2 != 1 ? qw : c.vcap;  // inverted-index entries per row (upper bound)
    p.irow = o; o = align_up(o + N * inv * 4, 256);
    p.ival = o; o = align_up(o + N * inv * 2, 256);
    p.dlist = o; o = align_up(o + N * 4, 256);
    p.dcount = o; o = align_up(o + 16, 256);
    p.krslab = o; o = align_up(o + (c.kr_fast ? 0 : GEN_WG * p.kr.bytes), 256);
    p.qeslab = o; o = align_up(o + (k2 != 1 ? GEN_WG * p.qe.bytes : 0), 256);
    p.total = o;
    return p;
}

// od rows: OD (N x N, row i = distances from item i, scaled by 1/rowdiv[i] on the fly).
static int rerank_core(const float* OD, int64_t N, int64_t Q, int k1, int k2, uint16_t lam16, float lam_f,
                       float* out, int64_t ldo, char* ws, const RrPlan& P, int32_t* flags, hipStream_t s) {
    const RrCaps& c = P.caps;
    float* rmax = (float*)(ws + P.rowmax);
    int32_t* R = (int32_t*)(ws + P.rank);
    int rc;
    if ((rc = rowmax_launch(OD, N, N, N, rmax, s))) return rc;
    if ((rc = topk_launch(OD, N, N, N, rmax, c.K, R, nullptr, c.K, s))) return rc;
    int32_t* vcol = (int32_t*)(ws + P.vcol);
    uint16_t* vval = (uint16_t*)(ws + P.vval);
    int32_t* vnnz = (int32_t*)(ws + P.vnnz);
    const DistSrc ds{OD, N, 0, nullptr, 0, 0, nullptr};
    if ((rc = v_rows_launch(ds, rmax, R, c.K, 0, N, c, ws + P.krslab, vcol, vval, vnnz, flags, s))) return rc;
    const Rows V = ell_rows(vnnz, c.vcap, vcol, vval);
    Rows Vq = V;  // (k2 = 1: V_qe = V)
    if (k2 != 1) {
        int32_t* qcol = (int32_t*)(ws + P.qcol);
        uint16_t* qval = (uint16_t*)(ws + P.qval);
        int32_t* qnnz = (int32_t*)(ws + P.qnnz);
        int32_t* dlist = (int32_t*)(ws + P.dlist);
        int32_t* dcount = (int32_t*)(ws + P.dcount);
        const bool fast = c.k2e <= QE_FAST_K2;
        if (fast) {
            if ((rc = qe_rows_launch(R, (int64_t)c.K, c.k2e, (int64_t)0, N, V, qcol, qval, qnnz, c.qcap, dlist, dcount, s)))
                return rc;
        }
        // the rows qe_kernel deferred (or every row): their count is read on the device
        if ((rc = qe_generic_launch(R, (int64_t)c.K, c.k2e, (int64_t)0, V, fast ? (const int32_t*)dlist : nullptr,
                                    fast ? (const int32_t*)dcount : nullptr, N, GEN_WG, 2, qcol, qval, qnnz, c.qcap,
                                    (const int64_t*)nullptr, P.qe, ws + P.qeslab, c.tcap, flags, s)))
            return rc;
        Vq = ell_rows(qnnz, c.qcap, qcol, qval);
    }
    int64_t* off = (int64_t*)(ws + P.off);
    int32_t* irow = (int32_t*)(ws + P.irow);
    uint16_t* ival = (uint16_t*)(ws + P.ival);
    if ((rc = csc_build(Vq, N, (int32_t*)(ws + P.cnt), (int32_t*)(ws + P.cur), off, irow, ival, s))) return rc;
    return jaccard_scan_launch(OD, N, rmax, Q, N, Vq, off, irow, ival, lam16, lam_f, out, ldo, s);
}

}  // namespace reidmi

using namespace reidmi;

// from_dist = 0: reidmi_rerank (distance computed inside); 1: reidmi_rerank_from_dist with
// need_transpose = (!symmetric || add != NULL).
REIDMI_API int64_t reidmi_rerank_workspace_bytes(int64_t Q, int64_t G, int k1, int k2, int from_dist,
                                                 int need_transpose) {
    const int64_t N = Q + G;
    if (Q < 0 || G < 0 || N <= 0 || k1 < 1 || k2 < 1) return -1;
    return rr_plan(N, k1, k2, !from_dist, from_dist && need_transpose).total;
}

REIDMI_API int reidmi_rerank(const float* feat, int64_t Q, int64_t G, int64_t D, int64_t ldf, int k1, int k2,
                             uint16_t one_minus_lambda_h, float lambda_f, float* final_dist, int64_t ldo, void* ws_,
                             int64_t ws_bytes, int32_t* flags, void* stream) {
    const int64_t N = Q + G;
    RM_REQUIRE(Q >= 0 && G >= 0 && N > 0 && D > 0 && ldf >= D && ldo >= G && flags && k1 >= 1 && k2 >= 1,
               "rerank: bad arguments");
    RM_REQUIRE(N < 0x7fffffff, "rerank: too many items");
    const RrPlan P = rr_plan(N, k1, k2, true, false);
    RM_REQUIRE(ws_bytes >= P.total, "rerank: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)ws_;
    float* Dm = (float*)(ws + P.dist);
    int rc;
    // R1: exact-fp32 distance over cat(q, g); symmetric bit-for-bit (computed as the upper
    // triangle + its mirror), so od rows = D rows
    if ((rc = distmat_self_launch(feat, N, ldf, D, Dm, N, Dm + N * N, s))) return rc;
    return rerank_core(Dm, N, Q, k1, k2, one_minus_lambda_h, lambda_f, final_dist, ldo, ws, P, flags, s);
}

REIDMI_API int reidmi_rerank_from_dist(const float* dist, const float* add, int64_t Q, int64_t G, int symmetric,
                                       int k1, int k2, uint16_t one_minus_lambda_h, float lambda_f, float* final_dist,
                                       int64_t ldo, void* ws_, int64_t ws_bytes, int32_t* flags, void* stream) {
    const int64_t N = Q + G;
    RM_REQUIRE(Q >= 0 && G >= 0 && N > 0 && ldo >= G && flags && k1 >= 1 && k2 >= 1,
               "rerank_from_dist: bad arguments");
    const bool need_t = !symmetric || add != nullptr;
    const RrPlan P = rr_plan(N, k1, k2, false, need_t);
    RM_REQUIRE(ws_bytes >= P.total, "rerank_from_dist: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)ws_;
    const float* OD = dist;
    if (need_t) {
        float* T = (float*)(ws + P.tdist);
        int rc;
        if ((rc = transpose_launch(dist, add, N, T, s))) return rc;
        OD = T;
    }
    return rerank_core(OD, N, Q, k1, k2, one_minus_lambda_h, lambda_f, final_dist, ldo, ws, P, flags, s);
}
