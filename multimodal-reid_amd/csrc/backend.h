// backend.h — the retrieval back end's internal launchers that another source calls, grouped by
// the file that defines them (internal, not part of the C ABI).  Callers: the distance launchers
// from rerank.hip (one-call R1), rerank_rank.hip (R2 chunks) and rerank_jaccard.hip (od chunks),
// the row norms from distance.h's dm_norms and cluster.hip; topk_launch from rerank.hip and rerank_rank.hip;
// evalfeat.hip its last stage; prefilter.hip's from rerank_rank.hip alone.  The re-rank sources'
// own cross-file launchers are in rerank.h.
#pragma once
#include "common.h"

namespace reidmi {

// distance.hip
void rows_sqnorm_launch(const float* x, int64_t n, int64_t d, int64_t ld, float* out, hipStream_t s);
int distmat_self_launch(const float* x, int64_t N, int64_t ldx, int64_t D, float* out, int64_t ldo, float* ws,
                        hipStream_t s);
int distmat_launch(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                   float* out, int64_t ldo, float* ws, hipStream_t s);
int distmat_pre_launch(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                       const float* qq, const float* gg, float* out, int64_t ldo, hipStream_t s);

// search.hip
int topk_launch(const float* x, int64_t rows, int64_t cols, int64_t ldx, const float* row_div, int k,
                int32_t* out_idx, float* out_val, int64_t ldo, hipStream_t s);

// eval.hip (the last stage of evalfeat.hip: it uses eval.hip's AP summers)
int evf_finish_launch(const int32_t* pos_cnt, int32_t* hist, const int32_t* junk_cnt, int64_t Q, int cap,
                      int64_t G_total, int32_t* overflow, int32_t* valid, int64_t* first, int64_t* last,
                      int32_t* npos, double* ap, int64_t* nkept, hipStream_t s);

// prefilter.hip
int rank_select_launch(float* dot, int64_t ldd, const float* feat, int64_t ldf, int D, const float* sqn,
                       const float* nrm, const float* nmax2, int64_t row0, int64_t rows, int64_t N, int K,
                       int32_t* rank_out, float* rowmax_out, int32_t* need, hipStream_t s);
void rank_select_consts(int D, float c[3]);
int norm_max_launch(const float* sqn, const float* nrm, int64_t N, float* out2, hipStream_t s);
int rr_sample_launch(const float* hs, int64_t lds, int64_t ns, const float* sqn, const float* nrm, const float* nmax2,
                     int64_t row0, int64_t rows, int K, int D, float4* meta, float* wrow, int32_t* cnt, int cap,
                     hipStream_t s);
int rank_select_sv_launch(const int32_t* cnt, const int2* list, int cap, const float* wrow, const float* feat,
                          int64_t ldf, int D, const float* sqn, int64_t row0, int64_t rows, int K, int32_t* rank_out,
                          float* rowmax_out, int32_t* need, hipStream_t s);
int feat16_launch(const float* x, int64_t N, int64_t D, int64_t ldx, void* y, int64_t Np, int64_t Dp,
                  int32_t* range_ok, hipStream_t s);

}  // namespace reidmi
