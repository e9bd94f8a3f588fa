// distance.hip — row norms and the exact fp32 distance matrix of the CLIP-ReID eval path on gfx950.
//
//   reidmi_row_sqnorm_f32  squared row norms (the distance's ||.||^2)   evaluate.py:10-11
//   reidmi_l2norm_f32      F.normalize(feats, p=2, dim=1)               evaluate.py:114
//   reidmi_distmat_f32     ||q||^2 + ||g||^2 - 2 q.g  (exact fp32)      evaluate.py:7-13, reranking.py:36-41
//   reidmi_cosine_f32      arccos of the clipped cosine similarity      evaluate.py:16-26
//
// The tile (mainloops, accumulator layout, distance value) and the bit-exact contract are in
// distance.h, shared with search.hip; the kernels, their store epilogue and launchers are here.
#include "backend.h"
#include "distance.h"
#include "rownorm.h"

namespace reidmi {

// --------------------------------------------------------------------------- norms
// R rows per R-thread workgroup, one row's fmaf chain per thread (k ascending, the distance
// kernel's arithmetic).  With 16-byte rows the row segments are staged through LDS 32 columns
// at a time by coalesced float4 loads (the next segment in flight while the current one is
// summed), instead of each thread walking its own row (uncoalesced).  R = 64: a Market gallery
// (15 913 rows) is 249 workgroups, not 63 on 256 CUs (rows_sqnorm_launch).
constexpr int RSQ_K = 32, RSQ_R = 64;
template <int R>
__global__ __launch_bounds__(R) void row_sqnorm_kernel(const float* __restrict__ x, int64_t n, int64_t d, int64_t ld,
                                                       float* __restrict__ out) {
    __shared__ float tile[R][RSQ_K + 1];
    const int64_t r0 = (int64_t)blockIdx.x * R, i = r0 + threadIdx.x;
    if ((ld & 3) != 0 || ((uintptr_t)x & 15) != 0 || d < RSQ_K) {  // uniform
        if (i >= n) return;
        const float* r = x + i * ld;
        float acc = 0.0f;
        for (int64_t k = 0; k < d; k++) acc = l2_sq_step(acc, r[k]);
        out[i] = acc;
        return;
    }
    // float4 f = threadIdx.x + R u of a segment: row f / 8, columns 4 (f % 8) .. + 3
    constexpr int U = RSQ_K / 4;
    float4 v[U];
    auto load = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int f = threadIdx.x + R * u, row = f >> 3, c = (f & 7) * 4;
            const int64_t gi = r0 + row < n ? r0 + row : n - 1;
            v[u] = *(const float4*)(x + gi * ld + k0 + c);
        }
    };
    const int64_t nk = d / RSQ_K;
    float acc = 0.0f;
    load(0);
    for (int64_t kt = 0; kt < nk; kt++) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int f = threadIdx.x + R * u, row = f >> 3, c = (f & 7) * 4;
            tile[row][c] = v[u].x;
            tile[row][c + 1] = v[u].y;
            tile[row][c + 2] = v[u].z;
            tile[row][c + 3] = v[u].w;
        }
        __syncthreads();
        if (kt + 1 < nk) load((kt + 1) * RSQ_K);
#pragma unroll
        for (int k = 0; k < RSQ_K; k++) acc = l2_sq_step(acc, tile[threadIdx.x][k]);
        __syncthreads();
    }
    if (i >= n) return;
    const float* r = x + i * ld;
    for (int64_t k = nk * RSQ_K; k < d; k++) acc = l2_sq_step(acc, r[k]);
    out[i] = acc;
}

void rows_sqnorm_launch(const float* x, int64_t n, int64_t d, int64_t ld, float* out, hipStream_t s) {
    hipLaunchKernelGGL(row_sqnorm_kernel<RSQ_R>, dim3((unsigned)ceil_div(n, RSQ_R)), dim3(RSQ_R), 0, s, x, n, d, ld,
                       out);
}

// y = x / max(sqrt(ss), 1e-12) (rownorm.h): one workgroup per row, coalesced.
__global__ void row_scale_kernel(const float* __restrict__ x, const float* __restrict__ ss, int64_t d,
                                 int64_t ldx, float* __restrict__ y, int64_t ldy) {
    int64_t i = blockIdx.x;
    const float den = l2_denominator(ss[i]);
    for (int64_t k = threadIdx.x; k < d; k += blockDim.x) y[i * ldy + k] = l2_scale(x[i * ldx + k], den);
}

// Store epilogue of the distance kernels.  SYM (the self-distance, q == g): also the mirrored tile.
template <bool COSINE, bool SYM>
__device__ __forceinline__ void dm_store_tile(const DmThread& t, const f32x16 (&acc)[2][2], const float* qq,
                                              const float* gg, int64_t Q, int64_t G, int64_t bm, int64_t bn,
                                              float* out, int64_t ldo) {
    const int lane = t.lane, wm = t.wm, wn = t.wn;
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int64_t i = bm + dm_lane_row(wm, mt, r, lane);
                const int64_t j = bn + dm_lane_col(wn, nt, lane);
                if (i < Q && j < G) {
                    if constexpr (COSINE) {
                        // evaluate.py:16-26: arccos(clip(q.g * (1/(|q||g|)), -1+1e-5, 1-1e-5))
                        const float c = acc[mt][nt][r] * (1.0f / (__builtin_sqrtf(qq[i]) * __builtin_sqrtf(gg[j])));
                        out[i * ldo + j] = acosf(fminf(fmaxf(c, -1.0f + 1e-5f), 1.0f - 1e-5f));
                    } else {
                        const float v = dm_value(acc[mt][nt][r], qq[i], gg[j]);
                        out[i * ldo + j] = v;
                        if (SYM && bm != bn) out[j * ldo + i] = v;  // the mirrored tile
                    }
                }
            }
}

template <bool COSINE>
__global__ __launch_bounds__(256) void distmat_f32_kernel(
    const float* __restrict__ q, const float* __restrict__ g, const float* __restrict__ qq,
    const float* __restrict__ gg, int64_t Q, int64_t G, int64_t D, int64_t ldq, int64_t ldg,
    float* __restrict__ out, int64_t ldo) {
    __shared__ float sA[DM_BK][DM_BM + DM_PAD];
    __shared__ float sB[DM_BK][DM_BN + DM_PAD];
    const DmThread t = dm_thread();
    const int64_t bm = (int64_t)blockIdx.y * DM_BM, bn = (int64_t)blockIdx.x * DM_BN;
    f32x16 acc[2][2];
    dm_acc_zero(acc);
    const int tid = threadIdx.x;
    for (int64_t k0 = 0; k0 < D; k0 += DM_BK) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            int e = tid + 256 * u;
            int r = e >> 4, kk = e & 15;
            int64_t gk = k0 + kk;
            int64_t qi = bm + r, gj = bn + r;
            sA[kk][r] = (qi < Q && gk < D) ? q[qi * ldq + gk] : 0.0f;
            sB[kk][r] = (gj < G && gk < D) ? g[gj * ldg + gk] : 0.0f;
        }
        __syncthreads();
        dm_kstep<DM_BK>(t, sA, sB, acc);
        __syncthreads();
    }
    dm_store_tile<COSINE, false>(t, acc, qq, gg, Q, G, bm, bn, out, ldo);
}

template <bool COSINE, bool SYM = false>
__global__ __launch_bounds__(256, DM2_MINWG) void distmat2_f32_kernel(
    const float* __restrict__ q, const float* __restrict__ g, const float* __restrict__ qq,
    const float* __restrict__ gg, int64_t Q, int64_t G, int64_t D, int64_t ldq, int64_t ldg,
    float* __restrict__ out, int64_t ldo) {
    __shared__ float sA[2][DM2_BK][DM2_LD];
    __shared__ float sB[2][DM2_BK][DM2_LD];
    // consecutive tiles, row tile fastest, so the row tiles of one gallery panel run back to back
    // on one XCD and its panel is fetched into that L2 once
    const int64_t tiles_m = (Q + DM_BM - 1) / DM_BM;
    const int64_t wg = xcd_contiguous_wg();
    int64_t bm, bn;
    if constexpr (SYM) {
        // the self-distance of one row set (q == g): tiles (tm, tn) with tm <= tn only, column
        // panel tn holding tiles 0..tn (tn (tn + 1) / 2 tiles before it); the epilogue also
        // writes the mirrored tile.  Bit-for-bit symmetric: fma(a, b, c) == fma(b, a, c) in
        // every step of the chain, and qq[i] + gg[j] == qq[j] + gg[i] (same array).
        int64_t tn = (int64_t)((__builtin_sqrt(8.0 * (double)wg + 1.0) - 1.0) * 0.5);
        while ((tn + 1) * (tn + 2) / 2 <= wg) tn++;
        while (tn * (tn + 1) / 2 > wg) tn--;
        bm = (wg - tn * (tn + 1) / 2) * DM_BM;
        bn = tn * DM_BN;
    } else if (DM2_BAND > 0 && tiles_m > DM2_BAND) {
        // bands of DM2_BAND row tiles walked column-major: the tiles an XCD runs at once
        // form a DM2_BAND x (32 / DM2_BAND) block, so their output rows are few and long
        const int64_t per = (int64_t)DM2_BAND * ((G + DM_BN - 1) / DM_BN), band = wg / per, r = wg - band * per;
        const int64_t rows = tiles_m - band * DM2_BAND < DM2_BAND ? tiles_m - band * DM2_BAND : DM2_BAND;
        bm = (band * DM2_BAND + r % rows) * DM_BM;
        bn = (r / rows) * DM_BN;
    } else {
        bm = (wg % tiles_m) * DM_BM;
        bn = (wg / tiles_m) * DM_BN;
    }
    const DmThread t = dm_thread();
    f32x16 acc[2][2];
    dm_acc_zero(acc);
    dm_tile_pipe(t, q, g, Q, G, D, ldq, ldg, bm, bn, sA, sB, acc);
    dm_store_tile<COSINE, SYM>(t, acc, qq, gg, Q, G, bm, bn, out, ldo);
}

// The one pick and launch of the distance kernel, norms given: the pipelined kernel when the
// operands allow (variant 1 forces the single-stage one), for sym (q == g, Q == G) its
// upper-triangle form.
static int distmat_dispatch(bool cosine, bool sym, int variant, const float* q, int64_t Q, int64_t ldq, const float* g,
                            int64_t G, int64_t ldg, int64_t D, const float* qq, const float* gg, float* out,
                            int64_t ldo, hipStream_t s) {
    const bool pipe = dm2_ok(q, ldq, g, ldg, D) && variant != 1;
    auto launch = [&](auto kernel, dim3 grid) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, q, g, qq, gg, Q, G, D, ldq, ldg, out, ldo);
    };
    if (sym && pipe) {
        const int64_t T = (Q + DM_BM - 1) / DM_BM;
        const int64_t tiles = T * (T + 1) / 2;
        RM_REQUIRE(tiles < (1ll << 31), "distmat_self: too many tiles");
        launch(distmat2_f32_kernel<false, true>, dim3((unsigned)tiles));
    } else {
        const dim3 grid(ceil_div(G, DM_BN), ceil_div(Q, DM_BM));
        RM_REQUIRE(grid.y <= 65535, "distmat: too many query rows for one launch");
        const dim3 grid1((unsigned)((int64_t)grid.x * grid.y));
        if (cosine) {
            if (pipe) launch(distmat2_f32_kernel<true>, grid1);
            else launch(distmat_f32_kernel<true>, grid);
        } else {
            if (pipe) launch(distmat2_f32_kernel<false>, grid1);
            else launch(distmat_f32_kernel<false>, grid);
        }
    }
    RM_LAUNCHED();
    return OK;
}

// ws: Q + G floats (the squared row norms).  variant: reidmi_distmat_f32_variant.
int distmat_impl(bool cosine, const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                 int64_t D, float* out, int64_t ldo, float* ws, void* stream, int variant = 0) {
    RM_REQUIRE(variant == 0 || variant == 1, "distmat variant: 0 auto, 1 single-stage");
    RM_REQUIRE(Q >= 0 && G >= 0 && D > 0 && ldq >= D && ldg >= D && ldo >= G, "distmat: bad shape");
    RM_REQUIRE(ws != nullptr, "distmat: workspace (Q+G floats) required");
    if (Q == 0 || G == 0) return OK;
    hipStream_t s = (hipStream_t)stream;
    float* qq = ws;
    float* gg = ws + Q;
    rows_sqnorm_launch(q, Q, D, ldq, qq, s);
    RM_LAUNCHED();
    rows_sqnorm_launch(g, G, D, ldg, gg, s);
    RM_LAUNCHED();
    return distmat_dispatch(cosine, false, variant, q, Q, ldq, g, G, ldg, D, qq, gg, out, ldo, s);
}

int distmat_launch(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                   float* out, int64_t ldo, float* ws, hipStream_t s) {
    return distmat_impl(false, q, Q, ldq, g, G, ldg, D, out, ldo, ws, s);
}

// Euclidean distance with precomputed squared row norms qq[Q], gg[G] (row_sqnorm_kernel).
int distmat_pre_launch(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                       const float* qq, const float* gg, float* out, int64_t ldo, hipStream_t s) {
    RM_REQUIRE(Q >= 0 && G >= 0 && D > 0 && ldq >= D && ldg >= D && ldo >= G && qq && gg, "distmat: bad shape");
    if (Q == 0 || G == 0) return OK;
    return distmat_dispatch(false, false, 0, q, Q, ldq, g, G, ldg, D, qq, gg, out, ldo, s);
}

// Self-distance of x [N][D] (the one-call re-rank's N x N matrix, reranking.py:36-44): the
// upper-triangle tiles and their mirror images, half the FLOPs of distmat_launch(x, x), same
// bits.  ws: N floats.
int distmat_self_launch(const float* x, int64_t N, int64_t ldx, int64_t D, float* out, int64_t ldo, float* ws,
                        hipStream_t s) {
    RM_REQUIRE(N > 0 && D > 0 && ldx >= D && ldo >= N && ws != nullptr, "distmat_self: bad shape");
    rows_sqnorm_launch(x, N, D, ldx, ws, s);
    RM_LAUNCHED();
    return distmat_dispatch(false, true, 0, x, N, ldx, x, N, ldx, D, ws, ws, out, ldo, s);
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_row_sqnorm_f32(const float* x, int64_t n, int64_t d, int64_t ldx, float* out, void* stream) {
    RM_REQUIRE(n >= 0 && d >= 0 && ldx >= d, "row_sqnorm: bad shape");
    if (n == 0) return OK;
    rows_sqnorm_launch(x, n, d, ldx, out, (hipStream_t)stream);
    RM_LAUNCHED();
    return OK;
}

REIDMI_API int reidmi_l2norm_f32(const float* x, int64_t n, int64_t d, int64_t ldx, float* y, int64_t ldy,
                                 float* ws, void* stream) {
    RM_REQUIRE(n >= 0 && d > 0 && ldx >= d && ldy >= d && ws != nullptr, "l2norm: bad shape or workspace");
    if (n == 0) return OK;
    hipStream_t s = (hipStream_t)stream;
    rows_sqnorm_launch(x, n, d, ldx, ws, s);
    RM_LAUNCHED();
    hipLaunchKernelGGL(row_scale_kernel, dim3((unsigned)n), dim3(256), 0, s, x, ws, d, ldx, y, ldy);
    RM_LAUNCHED();
    return OK;
}

REIDMI_API int reidmi_distmat_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                  int64_t D, float* out, int64_t ldo, float* ws, void* stream) {
    return distmat_impl(false, q, Q, ldq, g, G, ldg, D, out, ldo, ws, stream);
}

#ifdef REIDMI_TOOLS
// Per-call kernel selection (tests / A-B timing; tools library, include/reidmi_tools.h):
// 0 = auto (pipelined when the operands allow), 1 = the single-stage kernel; the same MFMA
// chain per output (bit-identical).
REIDMI_API int reidmi_distmat_f32_variant(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G,
                                          int64_t ldg, int64_t D, float* out, int64_t ldo, float* ws, int variant,
                                          void* stream) {
    return distmat_impl(false, q, Q, ldq, g, G, ldg, D, out, ldo, ws, stream, variant);
}
#endif

REIDMI_API int reidmi_cosine_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                 int64_t D, float* out, int64_t ldo, float* ws, void* stream) {
    return distmat_impl(true, q, Q, ldq, g, G, ldg, D, out, ldo, ws, stream);
}
