// prefilter.h — the pieces of the fp16 pre-filter that its two users share: the re-rank's R2
// (prefilter.hip's selection kernels, rerank_rank.hip's drivers) and the pre-filtered search
// (search_prefilter.hip).  One definition each of the exact chain, the bound's width, the sample's
// geometry, and the launchers of the survivor GEMM's inputs (kernels in rerank_rank.hip).  The
// error model of the bound is written out above rank_select1_kernel in prefilter.hip; the bound's
// constants are backend.h's rank_select_consts.  Internal, not part of the C ABI.
#pragma once
#include "backend.h"

namespace reidmi {

// Survivor capacity per row of the rectangular forms, and the default sample stride.
constexpr int RR_SV_CAP = 4096;
constexpr int RR_SAMPLE_STRIDE = 16;

// The sample of N items at stride S: every S-th item, floor(N / S) of them rounded down to whole
// 256-column tiles of the GEMM (0: no sampled form).
inline int64_t rr_sv_ns(int64_t N, int S) { return S >= 2 ? N / S / 256 * 256 : 0; }

constexpr int DE_UNROLL = 16;

// sum_k a[k] b[k] as the distance kernel accumulates it: one fmaf chain over k ascending from +0.
// vec: both rows are 16-byte aligned (four elements per load; the chain is the same).
__device__ __forceinline__ float dot_chain(const float* __restrict__ a, const float* __restrict__ b, int D, bool vec) {
    float acc = 0.0f;
    int k = 0;
    if (vec) {
        // unrolled so that many row loads are in flight ahead of the (sequential) fma chain
#pragma unroll DE_UNROLL
        for (; k + 4 <= D; k += 4) {
            const float4 x = *(const float4*)(a + k), y = *(const float4*)(b + k);
            acc = __builtin_fmaf(x.x, y.x, acc);
            acc = __builtin_fmaf(x.y, y.y, acc);
            acc = __builtin_fmaf(x.z, y.z, acc);
            acc = __builtin_fmaf(x.w, y.w, acc);
        }
    }
    for (; k < D; k++) acc = __builtin_fmaf(a[k], b[k], acc);
    return acc;
}

// The exact fp32 distance of items i and c of one feature set (16-byte aligned base): the distance
// kernel's bits, fma(-2, chain, s_i + s_c).
__device__ __forceinline__ float dist_exact(const float* __restrict__ feat, int64_t ldf, int D,
                                            const float* __restrict__ sqn, int64_t i, int64_t c) {
    return __builtin_fmaf(-2.0f, dot_chain(feat + i * ldf, feat + c * ldf, D, (ldf & 3) == 0), sqn[i] + sqn[c]);
}

__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) m = fmaxf(m, red[w]);
    __syncthreads();
    return m;
}

// Width of the pair bound of row i: hi(i, j) - (exact distance lower bound) <= w_i for every j,
// from the largest norm and squared norm over the items (e is increasing in both; the margin
// covers the roundings of hi, of fl(dt - e) and of this subtraction, each <= 2^-24 of
// magnitudes <= 2.2 (s_i + s_max)).  For L2-normalised features (every n_j = 1) it is 2 e + a
// few ulps, the width of the per-pair bound.
__device__ __forceinline__ float rr_width(float s_i, float n_i, float n_max, float s_max, float c_rel, float c_abs,
                                          float c_d) {
    const float e = 1.01f * (__builtin_fmaf(c_rel * n_i, n_max, 0x1p-23f * (s_i + s_max)) + c_abs * (n_i + n_max) + c_d);
    return 2.0f * e * (1.0f + 0x1p-10f) + 0x1p-20f * (s_i + s_max + e);
}

// The survivor epilogue's hi_max of a row with width w whose candidates are the pairs with
// lo = fl(hi - w) <= T: it bounds every such hi from above (the widening covers the roundings of
// hi - w and of T + w).  T finite.
__device__ __forceinline__ float rr_hmax(float T, float w) {
    return (T + w) + (fabsf(T) + w) * 0x1p-20f + 1e-37f;
}

// rerank_rank.hip: the inputs and the launch of the sampled forms' two GEMMs.
// sqn_s / nrm_s [ns] = sqn / nrm of every S-th item
int rr_gather_norms_launch(const float* sqn, const float* nrm, int64_t ns, int S, float* sqn_s, float* nrm_s,
                           hipStream_t s);
// the survivor epilogue's column records of the rectangular form: (s_c, n_c, 0, 0), zero past N; out [Np] float4
int rr_colrec_launch(const float* sqn, const float* nrm, int64_t N, int64_t Np, void* out, hipStream_t s);
// the tile list of a tm x tn rectangle in band order (gemm.h rr_tiles); out [tm * tn]
int rr_rect_tiles_launch(int tm, int tn, int* out, hipStream_t s);
// EPI_RRHI of rows a16 [nb][Dp] (row r is item row0 + r of rsqn / rnrm) against the sample w16 (row
// pitch ldw: every S-th item) with the sample's norms: hs [nb][ns] fp32 = hi
int rr_hi_sample_launch(const void* a16, int64_t Dp, const void* w16, int64_t ldw, const float* rsqn,
                        const float* rnrm, int64_t row0, int64_t nb, const float* sqn_s, const float* nrm_s,
                        int64_t ns, int64_t D, float* hs, hipStream_t s);
// EPI_RRSV of rows a16 [M][Dp] against w16 [Np][Dp] (N items) over a tile list: appends to cnt [M] /
// list [M][cap] (int2); tri: a16 = w16, the list is (part of) the upper triangle and each pair
// above the diagonal is tested for both its rows
int rr_survivors_launch(const void* a16, const void* w16, int64_t Dp, int64_t Np, int64_t N, int64_t D, int64_t M,
                        const void* rowmeta, const void* colrec, const int* tiles, int64_t ntiles, bool tri,
                        int32_t* cnt, void* list, int cap, hipStream_t s);

}  // namespace reidmi
