// distance.h — the exact fp32 distance tile, ||q||^2 + ||g||^2 - 2 q.g (evaluate.py:7-13,
// reranking.py:36-41), shared by the distance kernels (distance.hip) and the kernels that walk
// the tile over a query band and a gallery range without storing it (search.hip, evalfeat.hip,
// pairhist.hip, cluster.hip).  Device code, and the host side of the walk: the predicate that
// picks the mainloop, the launch plan, the norms at the head of the workspace; internal.
//
// Bit-exact contract with oracle/reid_oracle.c: every dot product / squared norm is an
// fmaf chain over k ascending.  The distance GEMM runs on v_mfma_f32_32x32x2_f32, whose
// result is bit-for-bit that chain (one rounding per product, k-pairs in order).
#pragma once
#include "backend.h"

namespace reidmi {

// ------------------------------------------------------------------- distance GEMM
// 128x128 output tile per 256-thread workgroup (2x2 waves, 64x64 per wave as 2x2
// 32x32 MFMA tiles).  Operands staged k-major in LDS so each MFMA operand read is 32
// consecutive floats per half-wave.  The dm_* functions below are the one definition of the
// tile (mainloops, accumulator layout, the distance value) that the distance kernels
// (distance.hip, with their store epilogue dm_store_tile) and the fused search
// (search.hip search_f32_kernel) share.
constexpr int DM_BM = 128, DM_BN = 128, DM_BK = 16, DM_PAD = 4;

// A thread's place in the workgroup's tile: wave wid = 2 wm + wn owns the 64x64 quadrant (wm, wn).
struct DmThread {
    int tid, lane, wid, wm, wn;
};
__device__ __forceinline__ DmThread dm_thread() {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    return {tid, lane, wid, wid >> 1, wid & 1};
}

// One staged K-step of the workgroup's tile: BK / 2 K-pairs ascending, four MFMAs each.  This
// is the only place the product is accumulated: per output the fmaf chain over k ascending.
template <int BK, int LD>
__device__ __forceinline__ void dm_kstep(const DmThread& t, const float (*sA)[LD], const float (*sB)[LD],
                                         f32x16 (&acc)[2][2]) {
    const int lane = t.lane, wm = t.wm, wn = t.wn;
#pragma unroll
    for (int s = 0; s < BK / 2; s++) {
        const int kr = 2 * s + (lane >> 5);
        const float a0 = sA[kr][wm * 64 + (lane & 31)];
        const float a1 = sA[kr][wm * 64 + 32 + (lane & 31)];
        const float b0 = sB[kr][wn * 64 + (lane & 31)];
        const float b1 = sB[kr][wn * 64 + 32 + (lane & 31)];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}

__device__ __forceinline__ void dm_acc_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = f32x16{};
}

// The tile functions add q[bm.., :] . g[bn.., :]^T to acc (the caller zeroes it) for the rows below
// Q and glim (the gallery's end, or the end of a search range); rows past them count as 0.  They
// read threadIdx.x for the staging index, not t.tid: with t.tid search_f32_kernel<true, false>
// spills 4 B more per lane.
// Single-stage mainloop (any D, pitch and alignment) of the search.  distmat_f32_kernel keeps its
// own copy of the staging loop around dm_kstep: through this function it ran 1.5 - 5 % slower
// (profiles/r08/distance_dedup_ab.txt).
__device__ __forceinline__ void dm_tile_single(const DmThread& t, const float* q, const float* g, int64_t Q,
                                               int64_t glim, int64_t D, int64_t ldq, int64_t ldg, int64_t bm,
                                               int64_t bn, float (*sA)[DM_BM + DM_PAD], float (*sB)[DM_BN + DM_PAD],
                                               f32x16 (&acc)[2][2]) {
    const int tid = threadIdx.x;
    for (int64_t k0 = 0; k0 < D; k0 += DM_BK) {
        // stage: 128 rows x 16 k per operand, 8 elements per thread, 16 threads per row
#pragma unroll
        for (int u = 0; u < 8; u++) {
            int e = tid + 256 * u;
            int r = e >> 4, kk = e & 15;
            int64_t gk = k0 + kk;
            int64_t qi = bm + r, gj = bn + r;
            sA[kk][r] = (qi < Q && gk < D) ? q[qi * ldq + gk] : 0.0f;
            sB[kk][r] = (gj < glim && gk < D) ? g[gj * ldg + gk] : 0.0f;
        }
        __syncthreads();
        dm_kstep<DM_BK>(t, sA, sB, acc);
        __syncthreads();
    }
}

// Pipelined mainloop (D, ldq, ldg multiples of 4, 16-byte aligned rows): K-step DM2_BK, two
// LDS stages, the next K-step's operands loaded as coalesced float4 into registers while the
// current one is multiplied, one barrier per K-step.
// LDS rows padded by 1 dword so the transposed scalar stores are conflict-free.  The MFMA
// sequence per output is dm_kstep's, as in dm_tile_single, so the result is bit-identical to it
// (and to the oracle's fmaf chain).  search_f32_kernel<true, *> keeps its own copy of this loop
// (its own four MFMAs included): through this function the labelled search ran 0.1 - 0.45 %
// slower than the copy's slowest run (profiles/r08/distance_dedup_ab.txt).
// K-step 16 (33 KB of LDS, 112 VGPRs): four workgroups per CU; K-step 32 ran two (66 KB) and
// was 5 % slower at MSMT17 / re-rank-chunk sizes (profiles/r02/distmat_kstep_ab.txt).  The
// macro is an A/B hook for tools/build_variant.py.
#ifndef DM2_BK_
#define DM2_BK_ 16
#endif
#if !defined(REIDMI_TOOLS) && DM2_BK_ != 16
#error "distance.h: DM2_BK_ variants build only with -DREIDMI_TOOLS (never into libreidmi.so)"
#endif
constexpr int DM2_BK = DM2_BK_, DM2_MINWG = 4, DM2_BAND = 4, DM2_LD = DM_BM + 1;
constexpr int DM2_F4 = DM2_BK / 4;            // float4 per operand row and K-step
constexpr int DM2_U = DM_BM * DM2_F4 / 256;   // float4 staging slots per thread and operand

__device__ __forceinline__ void dm_tile_pipe(const DmThread& t, const float* q, const float* g, int64_t Q,
                                             int64_t glim, int64_t D, int64_t ldq, int64_t ldg, int64_t bm,
                                             int64_t bn, float (*sA)[DM2_BK][DM2_LD], float (*sB)[DM2_BK][DM2_LD],
                                             f32x16 (&acc)[2][2]) {
    const int tid = threadIdx.x;
    // staging slots: float4 f = tid + 256u -> row f / DM2_F4, k group (f % DM2_F4) * 4
    const float* pa[DM2_U];
    const float* pb[DM2_U];
    bool va[DM2_U], vb[DM2_U];
    int srow[DM2_U], sk[DM2_U];
#pragma unroll
    for (int u = 0; u < DM2_U; u++) {
        const int f = tid + 256 * u;
        srow[u] = f / DM2_F4;
        sk[u] = (f % DM2_F4) * 4;
        va[u] = bm + srow[u] < Q;
        vb[u] = bn + srow[u] < glim;
        pa[u] = q + (va[u] ? bm + srow[u] : 0) * ldq + sk[u];
        pb[u] = g + (vb[u] ? bn + srow[u] : 0) * ldg + sk[u];
    }
    float4 ra[DM2_U], rb[DM2_U];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < DM2_U; u++) {
            const bool kin = k0 + sk[u] < D;  // D % 4 == 0: a float4 is wholly in or out
            ra[u] = va[u] && kin ? *(const float4*)(pa[u] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
            rb[u] = vb[u] && kin ? *(const float4*)(pb[u] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto lstore = [&](int st) {
#pragma unroll
        for (int u = 0; u < DM2_U; u++) {
            sA[st][sk[u] + 0][srow[u]] = ra[u].x;
            sA[st][sk[u] + 1][srow[u]] = ra[u].y;
            sA[st][sk[u] + 2][srow[u]] = ra[u].z;
            sA[st][sk[u] + 3][srow[u]] = ra[u].w;
            sB[st][sk[u] + 0][srow[u]] = rb[u].x;
            sB[st][sk[u] + 1][srow[u]] = rb[u].y;
            sB[st][sk[u] + 2][srow[u]] = rb[u].z;
            sB[st][sk[u] + 3][srow[u]] = rb[u].w;
        }
    };
    gload(0);
    lstore(0);
    __syncthreads();
    const int64_t nk = (D + DM2_BK - 1) / DM2_BK;
    for (int64_t kt = 0; kt < nk; kt++) {
        const int cur = (int)(kt & 1);
        if (kt + 1 < nk) gload((kt + 1) * DM2_BK);
        dm_kstep<DM2_BK>(t, sA[cur], sB[cur], acc);
        if (kt + 1 < nk) lstore(cur ^ 1);
        __syncthreads();
    }
}

// The accumulator layout of v_mfma_f32_32x32x2_f32: element r of acc[mt][nt] in this lane is
// row dm_lane_row, column dm_lane_col of the workgroup's tile (wm, wn: the wave's quadrant).
// search_f32_kernel's epilogue writes the same two expressions out (il, j): keep them in step.
__device__ __forceinline__ int dm_lane_row(int wm, int mt, int r, int lane) {
    return wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}
__device__ __forceinline__ int dm_lane_col(int wn, int nt, int lane) { return wn * 64 + nt * 32 + (lane & 31); }

// The distance: ||q||^2 + ||g||^2 - 2 q.g with one rounding in the sum of norms and one in the fma.
__device__ __forceinline__ float dm_value(float acc, float qq, float gg) { return __builtin_fmaf(-2.0f, acc, qq + gg); }

// 1-D grid, XCD-contiguous: workgroups bid, bid+8, ... share an XCD (round-robin dispatch) and
// get consecutive numbers, so what consecutive numbers share is fetched into that XCD's L2 once.
__device__ __forceinline__ int64_t xcd_contiguous_wg() {
    const int64_t nwg = (int64_t)gridDim.x;
    const int64_t bid = blockIdx.x, xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// ------------------------------------------------------------- the band-and-range walk
// The kernels that select, count or join in the tile's epilogue instead of storing it
// (search_f32_kernel, evf_count_kernel, ph_tile_kernel, dbs_tile_kernel) share one geometry: a
// 256-thread workgroup owns one 128-row query band and one contiguous gallery range [c0, c1) of
// range_len columns (whole tiles, unless a tool forces the ranges) and walks it in 128-column
// tiles.  The grid is bands x S workgroups, at most the DM_SLOTS resident ones (dm_walk_plan).

// Floats of LDS that hold the stages of either mainloop.
constexpr int DM_SMEM = 2 * 2 * DM2_BK * DM2_LD;
static_assert(DM_SMEM >= 2 * DM_BK * (DM_BM + DM_PAD), "dm_tile: both mainloops' stages fit");

// One tile by the mainloop the launcher picked (dm2_ok), its stages carved out of smem[DM_SMEM].
// Both mainloops end on a barrier: afterwards smem is free, for the next tile or the caller's use.
template <bool PIPE>
__device__ __forceinline__ void dm_tile(const DmThread& t, const float* q, const float* g, int64_t Q, int64_t glim,
                                        int64_t D, int64_t ldq, int64_t ldg, int64_t bm, int64_t bn, float* smem,
                                        f32x16 (&acc)[2][2]) {
    if constexpr (PIPE)
        dm_tile_pipe(t, q, g, Q, glim, D, ldq, ldg, bm, bn, (float(*)[DM2_BK][DM2_LD])smem,
                     (float(*)[DM2_BK][DM2_LD])(smem + 2 * DM2_BK * DM2_LD), acc);
    else
        dm_tile_single(t, q, g, Q, glim, D, ldq, ldg, bm, bn, (float(*)[DM_BM + DM_PAD])smem,
                       (float(*)[DM_BN + DM_PAD])(smem + DM_BK * (DM_BM + DM_PAD)), acc);
}

// This workgroup's place in the walk: band `band` (rows from bm) of `bands`, gallery range `split`
// = columns [c0, c1).  Band fastest: the bands of one gallery range get consecutive numbers, so
// they run side by side on one XCD and share the range's tiles in that L2.
struct DmWalk {
    int64_t bands, band, split, bm, c0, c1;
};
__device__ __forceinline__ DmWalk dm_walk(int64_t Q, int64_t G, int64_t range_len) {
    const int64_t bands = (Q + DM_BM - 1) / DM_BM;
    const int64_t wg = xcd_contiguous_wg();
    const int64_t band = wg % bands, split = wg / bands, bm = band * DM_BM;
    const int64_t c0 = split * range_len, c1 = c0 + range_len < G ? c0 + range_len : G;
    return {bands, band, split, bm, c0, c1};
}

// Person and camera ids of the query and the gallery rows (evaluate.py:46-48).  Which of them may
// be null is the entry point's contract.
struct DmLabels {
    const int64_t *qp, *qc, *gp, *gc;
};

// ---------------------------------------------------------------- the walk's host side
// The operands allow dm_tile_pipe (every launcher picks the mainloop by it).
inline bool dm2_ok(const float* q, int64_t ldq, const float* g, int64_t ldg, int64_t D) {
    return D % 4 == 0 && ldq % 4 == 0 && ldg % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)g & 15) == 0;
}

// The launch plan, a pure function of the shape: `tiles` gallery tiles cut into S ranges of
// range_len columns (whole tiles) so that bands x S workgroups fill, and do not exceed, the
// DM_SLOTS resident workgroups.  More bands than slots: one range per band.  No bands (Q == 0,
// nothing is launched): one range.  The caller checks bands * S < 2^31 under its own name.
constexpr int DM_SLOTS = 1024;  // 256 CUs x DM2_MINWG
inline void dm_walk_plan(int64_t bands, int64_t tiles, int64_t* S, int64_t* range_len) {
    int64_t s0 = bands > 0 ? DM_SLOTS / bands : 1;
    s0 = s0 < 1 ? 1 : (s0 > tiles ? tiles : s0);
    const int64_t per = (tiles + s0 - 1) / s0;
    *S = (tiles + per - 1) / per;
    *range_len = per * DM_BN;
}

// The head of every walk's workspace: the squared norms qq [Q] | gg [G], padded to 16 bytes.
inline int64_t dm_norm_bytes(int64_t Q, int64_t G) { return ((Q + G) * 4 + 15) / 16 * 16; }
inline int dm_norms(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D,
                    float* qq, float* gg, hipStream_t s) {
    rows_sqnorm_launch(q, Q, D, ldq, qq, s);
    RM_LAUNCHED();
    rows_sqnorm_launch(g, G, D, ldg, gg, s);
    RM_LAUNCHED();
    return OK;
}

}  // namespace reidmi
