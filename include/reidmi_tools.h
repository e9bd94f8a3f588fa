/*
 * reidmi_tools.h — entry points of libreidmi_tools.so only: the product library
 * (libreidmi.so, reidmi.h) plus the forced-variant calls that tests and A/B tools use to
 * check that every kernel choice gives the same bits and to time one choice against another.
 * None of them is on the product path: the product library is built without them
 * (REIDMI_TOOLS undefined), and multimodal_reid_amd._lib.load_tools() loads this one.
 */
#ifndef REIDMI_TOOLS_H
#define REIDMI_TOOLS_H
#include "reidmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* reidmi_distmat_f32 with an explicit kernel choice (no process-global state): variant 0 =
 * auto (K-step-32 pipelined kernel when D, ldq, ldg are multiples of 4 and the operands 16-byte
 * aligned), 1 = single-stage kernel.  Both run the same MFMA sequence per output: bit-identical. */
int reidmi_distmat_f32_variant(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                               int64_t D, float* out, int64_t ldo, float* ws, int variant, void* stream);

/* reidmi_search_f32 with a forced number of gallery ranges (splits: 1..min(G, 4096), ranges of
 * ceil(G / splits) columns, tile-aligned or not; 0 = the launcher's choice) and a forced
 * candidate-list capacity per row (k + 128 <= cap <= 512; 0 = the launcher's choice), so that
 * tests can make rows overflow and compact.  Every choice gives the same lists.  stats
 * (nullable, device int32[2], added to: zero it first): [0] the compactions a full list forced
 * (the one that sets a row's first threshold once it holds k candidates is not counted, nor the
 * final one), [1] the (distance, index) pairs the filter kept.  ws: at least
 * reidmi_search_ex_workspace_bytes(Q, G, D, k, splits, cap) bytes. */
int64_t reidmi_search_ex_workspace_bytes(int64_t Q, int64_t G, int64_t D, int k, int splits, int cap);
int reidmi_search_f32_ex(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                         int k, const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                         const int64_t* g_cams, int32_t* out_idx, float* out_dist, int64_t ldo, void* ws,
                         int64_t ws_bytes, int splits, int cap, int32_t* stats, void* stream);
/* reidmi_search_bounded_f32 with the same forced splits, capacity and counters: stats[1] counts
 * the pairs that passed the bound, the running threshold and the labels (0 when the bound admits
 * nothing: the filter runs before any append), stats[0] as above (the compaction after which a
 * bounded row's own k-th key replaces its bound is the uncounted first one). */
int reidmi_search_bounded_f32_ex(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                 int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams,
                                 const int64_t* g_pids, const int64_t* g_cams, const float* bound_dist,
                                 const int32_t* bound_idx, int64_t ldb, int64_t index_base, int32_t* out_idx,
                                 float* out_dist, int64_t ldo, void* ws, int64_t ws_bytes, int splits, int cap,
                                 int32_t* stats, void* stream);
/* reidmi_search_filtered_f32 with the same forced splits, capacity and counters (stats[1] counts
 * the pairs that also passed the filter's clauses). */
int reidmi_search_filtered_f32_ex(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                  int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams,
                                  const int64_t* g_pids, const int64_t* g_cams, const reidmi_search_filter* flt,
                                  const float* bound_dist, const int32_t* bound_idx, int64_t ldb, int64_t index_base,
                                  int32_t* out_idx, float* out_dist, int64_t ldo, void* ws, int64_t ws_bytes,
                                  int splits, int cap, int32_t* stats, void* stream);

/* reidmi_gemm_f16 with an explicit tiling: tile 0 = auto (the persistent 256x256x64 LDS-DMA
 * tile for >= 256 tiles, else 128x128x64), 1 = force 128x128, 2 = force persistent; ngroups =
 * the persistent walk's XCD groups (1, 2, 4, 8; each owns 1/ngroups of the N-tiles), 0 = auto.
 * Every choice is bit-identical. */
int reidmi_gemm_f16_tiled(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N,
                          int64_t K, const float* bias, const void* rowstat, const float* colsum, void* out,
                          int64_t ldc, int tile, int ngroups, void* stream);

/* One-wave-per-SIMD GEMM prototype (gemm_tools.hip gemm_w4_kernel): out fp16 = A.W^T + bias, same MFMA
 * chain as reidmi_gemm_f16 epi 0 (bit-identical); nostore: the values are computed, not stored.
 * N % 256 == 0, K % 64 == 0, K >= 128. */
int reidmi_gemm_f16_w4(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K,
                       const float* bias, void* out, int64_t ldc, int nostore, void* stream);

/* The round-robin vision attention kernel (mhsa_rr_kernel: 8 waves walk (head, 32-query block)
 * units over three LDS slots) for non-causal 205 <= L <= 212 with V^T rows of 212 elements:
 * bit-identical to reidmi_mhsa_f16 (which takes V^T rows of reidmi_attn_lpad(L)), measured no
 * faster, so only the tools library has it. */
int reidmi_mhsa_f16_rr(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H,
                       void* stream);

/* The single-query (CLS) attention of the last block's K / V path (mhsa_cls_kernel, one wave per
 * (sequence, head)): q [nseq*H][64] fp16 (the CLS rows), k [nseq*H][L][64] and vt [nseq*H][64][lpad]
 * as reidmi_mhsa_f16 takes them (lpad = reidmi_attn_lpad(L); columns >= L are never used, though
 * the 8-element piece holding column L-1 is read whole), 1 <= L <= 256 -> o [nseq][H*64] fp16. */
int reidmi_mhsa_cls_f16(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H,
                        void* stream);

/* The single-query (CLS) attention of the K / V path beyond 256 tokens (mhsa_cls_long_kernel:
 * the same arithmetic with the keys walked in chunks), 1 <= L <= 1024, vt rows of
 * reidmi_attn_vt_stride(L) (columns >= L never used; no piece is read past a row's end)
 * -> o [nseq][H*64] fp16. */
int reidmi_mhsa_cls_long_f16(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H,
                             void* stream);

/* The last block's CLS attention without K and V (cls_u_kernel, cls_attn_kernel, cls_o_kernel;
 * attention.hip): x [nseq*L][W] fp16 (the block's ln_1 input), rs [nseq*L][2] fp32 = (rstd, -mean
 * rstd) of its rows (reidmi_row_stats_f16), q [nseq][W] fp16 (the CLS queries, head-major), wqkv
 * [3W][W] fp16 / colsum [3W] / bias [3W] the ln_1-folded in_proj -> o [nseq][W] fp16.  W is 768 or
 * 1024 with H = W / 64, 1 <= L <= 224; nseq = 0 is a no-op.  Neither x nor rs needs padding: rows
 * past L of the last 32-token chunk re-read row L-1 of x (weight 0) and read no rs, images past
 * nseq of the last group of 16 re-read image nseq-1 and are not stored.  ws holds u, the score
 * constants, z and alpha: at least reidmi_cls_attn_nokv_ws_bytes(nseq, W) bytes (ws_bytes, checked),
 * 256-byte aligned. */
int64_t reidmi_cls_attn_nokv_ws_bytes(int64_t nseq, int W);
int reidmi_cls_attn_nokv_f16(const void* x, const void* rs, const void* q, const void* wqkv, const float* colsum,
                             const float* bias, int64_t nseq, int L, int H, int W, void* ws, int64_t ws_bytes, void* o,
                             void* stream);

/* The QKV GEMM alone (ln_1 fold + the head split reidmi_vit_forward uses): x [nseq*L][lda],
 * W [3*H*64][ldw] -> q, k [nseq*H][L][64], vt [nseq*H][64][lpad] (lpad = reidmi_attn_lpad(L)). */
int reidmi_gemm_f16_qkv(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t nseq, int L, int H,
                        const float* bias, const void* rowstat, const float* colsum, void* q, void* k, void* vt,
                        int lpad, void* stream);

/* reidmi_gemm_f16_qkv for columns [n_off, n_off + N) of [q | k | v] (n_off a multiple of 64; W, bias
 * and colsum point at the first of them) with an explicit tiling (tile, ngroups: as
 * reidmi_gemm_f16_tiled).  The outputs of column blocks the GEMM does not produce may be NULL:
 * n_off = H*64, N = 2*H*64 is the K / V-only GEMM, L = 1 with lpad = 1 and lda = the sequence stride
 * the CLS-query GEMM of the encoder's last block. */
int reidmi_gemm_f16_qkv_ex(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t nseq, int L, int H,
                           int64_t N, int64_t n_off, const float* bias, const void* rowstat, const float* colsum,
                           void* q, void* k, void* vt, int lpad, int tile, int ngroups, void* stream);

/* The pieces of reidmi_vit_forward / reidmi_text_forward between their GEMMs, each through the
 * launcher its tower runs.
 *
 * Patch columns: images [B][3][H][Wimg] (fp32, or fp16 with images_f16) -> col [B*gh*gw][kpad] fp16,
 * column c*patch^2 + ky*patch + kx, zero from 3*patch^2 on; tta (nullable) [B][2] = (top, left) of the
 * augmented view (flip, Pad((10,5)), crop).  The compile-time patch sizes (16, 14) run when kpad is
 * the packed round_up(3*patch^2, 64), else the runtime-patch kernel. */
int reidmi_im2col_f16(const void* images, int images_f16, int64_t B, int H, int Wimg, int patch, int stride, int gh,
                      int gw, int kpad, const int32_t* tta, void* col, void* stream);

/* Patch embed: x [B*L][W] fp16, L = 1 + NP + n_ctx: x[b*L+1+p] = col[b*NP+p] . conv_w^T + pos_emb[1+p]
 * (the conv1 GEMM's epilogue; conv_w [W][kpad] fp16, tile as reidmi_gemm_f16_tiled), x[b*L] =
 * class_emb + pos_emb[0], x[b*L+1+NP+i] = vpt[i]. */
int reidmi_patch_embed_f16(const void* col, const void* conv_w, const float* pos_emb, const float* class_emb,
                           const float* vpt, int n_ctx, int64_t B, int NP, int W, int kpad, void* x, int tile,
                           void* stream);

/* reidmi_layernorm on fp16 rows (the towers' residual stream; W in 512, 768, 1024): output row r
 * is LayerNorm(x[row_idx ? row_idx[r] : r]), written to any of y32 (fp32), y16 and yh (fp16; yh may
 * be x itself, the in-place ln_pre); sto (nullable, needs yh) [rows][2] receives (rstd, -mean*rstd)
 * of the fp16 rows written to yh, the bits reidmi_row_stats_f16 gives on them. */
int reidmi_layernorm_f16(const void* x, int64_t rows, int64_t ldx, const int32_t* row_idx, int64_t W,
                         const float* gamma, const float* beta, float eps, float* y32, int64_t ldy32, void* y16,
                         int64_t ldy16, void* yh, int64_t ldyh, void* sto, void* stream);

/* Text embed: x [N*L][W] fp16, x[n*L+t] = half((prompts ? prompts[n][t] : tok_emb[tokens[n][t]]) +
 * pos_emb[t]) for the first L of the Lt positions of tokens [N][Lt] (int64) / prompts [N][Lt][W];
 * rows[n] = n*L + min(argmax(tokens[n]) over all Lt positions (first maximum), L-1). */
int reidmi_text_embed_f16(const int64_t* tokens, const float* prompts, const float* tok_emb, const float* pos_emb,
                          int64_t N, int L, int Lt, int W, int64_t vocab, void* x, int32_t* rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REIDMI_TOOLS_H */
