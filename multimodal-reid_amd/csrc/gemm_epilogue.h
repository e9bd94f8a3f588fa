// gemm_epilogue.h — what the GEMM kernels share (gemm.hip's two tilings, the tools prototype
// of gemm_tools.hip): the tile constants, the A/B timing hooks, the small device helpers and
// the fused epilogues of the encoder and the re-rank bound (gemm.h Epi).  Device code only; it
// is compiled inside the kernels of the source that includes it.
#pragma once
#include "gemm.h"

namespace reidmi {

constexpr int GB_M = 128, GB_N = 128, GB_K = 64;
// the persistent 256x256 tile (gemm.hip; the prototype runs the same tile) and an LDS-DMA target
constexpr int G2_M = 256, G2_N = 256;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// Timing variants (tools/build_variant.py -D...=1; never set in the product or tools builds):
// epilogue pieces compiled out with their values kept live, to price each piece in A/B runs.
#ifndef GEMM_VAR_NOSTORE
#define GEMM_VAR_NOSTORE 0
#endif
#ifndef GEMM_VAR_NOGELU
#define GEMM_VAR_NOGELU 0
#endif
#ifndef GEMM_VAR_NOPSTAT
#define GEMM_VAR_NOPSTAT 0
#endif
#ifndef GEMM_VAR_NORESLOAD
#define GEMM_VAR_NORESLOAD 0
#endif
#ifndef GEMM_VAR_NODMA  // timing-only (wrong results): no operand DMA inside the K-loop
#define GEMM_VAR_NODMA 0
#endif
#ifndef GEMM_VAR_NOWAIT  // timing-only (racy results): no counted operand wait (vmcnt(6)) in the K-loop
#define GEMM_VAR_NOWAIT 0
#endif
#ifndef GEMM_VAR_ASAME  // timing-only (wrong results): every tile's A operand DMA reads row tile 0 (L2-resident)
#define GEMM_VAR_ASAME 0
#endif
// The A/B hooks above compile other kernels (the timing-only ones give wrong results by design):
// any value but the shipped one is refused outside a tools / variant build (-DREIDMI_TOOLS:
// libreidmi_tools.so, tools/build_variant.py), so none can enter libreidmi.so.
#if !defined(REIDMI_TOOLS) &&                                                                             \
    (GEMM_VAR_NOSTORE != 0 || GEMM_VAR_NOGELU != 0 || GEMM_VAR_NOPSTAT != 0 || GEMM_VAR_NORESLOAD != 0 || \
     GEMM_VAR_NODMA != 0 || GEMM_VAR_ASAME != 0 || GEMM_VAR_NOWAIT != 0)
#error "gemm.hip: GEMM_VAR_* variants build only with -DREIDMI_TOOLS (never into libreidmi.so)"
#endif

__device__ __forceinline__ int swz(int r, int kc) { return r * GB_K + ((kc ^ ((r >> 1) & 7)) << 3); }

typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// one v_cvt_pk_f16_f32 (RNE) per pair
__device__ __forceinline__ uint32_t cvt_pk_f16(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2v{a, b}, f16x2v));
}

// Two QuickGELUs, x * sigmoid(1.702 x) = x / (1 + 2^(-1.702 log2(e) x))
// (custom_clip_model.py:52-54), with the multiplies and the add on packed-fp32 VALU.
__device__ __forceinline__ f32x2v quick_gelu2(f32x2v x) {
    const f32x2v y = x * -2.4554669595930157f;
    const f32x2v d = f32x2v{__builtin_amdgcn_exp2f(y.x), __builtin_amdgcn_exp2f(y.y)} + 1.0f;
    return x * f32x2v{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
}

__device__ __forceinline__ f32x4 mfma16(const f16x8& w, const f16x8& a, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(w, a, c, 0, 0, 0);
}

// x[l] + x[l ^ 16] and x[l] + x[l ^ 32] by the VALU lane swaps (no LDS round trip, unlike
// __shfl_xor's ds_bpermute); fp32 addition is commutative, so the sums equal the shuffle's
// (results copied out as uint32_t before the bit_cast: attention.hip xhalf_pair)
__device__ __forceinline__ float xor16_sum(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    const auto p = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const uint32_t p0 = p[0], p1 = p[1];
    return __builtin_bit_cast(float, p0) + __builtin_bit_cast(float, p1);
}
__device__ __forceinline__ float xor32_sum(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    const auto p = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const uint32_t p0 = p[0], p1 = p[1];
    return __builtin_bit_cast(float, p0) + __builtin_bit_cast(float, p1);
}

// LayerNorm fold (see gemm.h EpiArgs) with the bias: acc <- rstd_m * acc + (-mean_m rstd_m
// * s_n + b'_n), two FMAs per element (bias b'_n of the lane's columns passed in bn).  Lane
// layout as epilogue_tile; rows past M read row M-1.
template <int NI>
__device__ __forceinline__ void ln_fold(f32x4 (&acc)[NI][4], const float2* __restrict__ rowstat,
                                        const float* __restrict__ colsum, const float4 (&bn)[4], int64_t mrow,
                                        int ncol, int64_t M) {
    const int lane = threadIdx.x & 63;
    const int cq = (lane >> 4) * 4;
    float4 sn[4];
#pragma unroll
    for (int j = 0; j < 4; j++) sn[j] = *(const float4*)(colsum + ncol + j * 16 + cq);
    float2 rs[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        int64_t m = mrow + i * 16 + (lane & 15);
        rs[i] = rowstat[m < M ? m : M - 1];
    }
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            acc[i][j][0] = __builtin_fmaf(rs[i].x, acc[i][j][0], __builtin_fmaf(rs[i].y, sn[j].x, bn[j].x));
            acc[i][j][1] = __builtin_fmaf(rs[i].x, acc[i][j][1], __builtin_fmaf(rs[i].y, sn[j].y, bn[j].y));
            acc[i][j][2] = __builtin_fmaf(rs[i].x, acc[i][j][2], __builtin_fmaf(rs[i].y, sn[j].z, bn[j].z));
            acc[i][j][3] = __builtin_fmaf(rs[i].x, acc[i][j][3], __builtin_fmaf(rs[i].y, sn[j].w, bn[j].w));
        }
}

// Epilogue of one wave's output block: NI row groups x 4 column groups of 16x16, lane
// holding C[m][nb..nb+3] with m = mrow + i*16 + (lane&15), nb = ncol + j*16 + (lane>>4)*4
// (see gemm.h for the modes).  All loads are hoisted ahead of the stores they feed: bias
// once per tile, residual rows all at once, pos-embed rows in batches — otherwise the
// compiler (which cannot prove `out` does not alias `bias`/`pos`) serialises one memory
// round trip per fragment.
// The residual epilogue's row reads: lane group q holds columns colp(jp) .. +7 of its row
// after the accumulator pairing below (rows past M read row M - 1; never stored).
template <int NI>
__device__ __forceinline__ void resid_rows_load(const EpiArgs& ea, int64_t mrow, int ncol, int64_t M,
                                                f16x8 (&xv)[NI][2]) {
    const int lane = threadIdx.x & 63, q = lane >> 4;
    const int64_t b0 = mrow < M ? mrow : M - 1;
    const char* const ob = (const char*)((const _Float16*)ea.out + b0 * ea.ldc);
#pragma unroll
    for (int i = 0; i < NI; i++) {
        int64_t m = mrow + i * 16 + (lane & 15);
        m = m < M ? m : M - 1;
#pragma unroll
        for (int jp = 0; jp < 2; jp++) {
            const int c = ncol + (2 * jp + (q & 1)) * 16 + (q >> 1) * 8;
            xv[i][jp] = *(const f16x8*)(ob + (uint32_t)((int)(m - b0) * (int)ea.ldc + c) * 2u);
        }
    }
}

// PRE: the residual rows were read by resid_rows_load into *xpre (EPI_RESID_F16 only);
// FULL: every row of the wave's block exists, so the fp16 path stores without per-row checks
template <int EPI, int NI, bool BIAS_DONE = false, bool PRE = false, bool FULL = false>
__device__ __forceinline__ void epilogue_tile(const EpiArgs& ea, f32x4 (&acc)[NI][4], int64_t mrow, int ncol,
                                              int64_t M, int N, const f16x8 (*xpre)[2] = nullptr) {
    const int lane = threadIdx.x & 63;
    const int cq = (lane >> 4) * 4;
    // fp16 output rows: a wave-uniform base row (the wave's first row, or the last row when the
    // wave has none) and per-lane 32-bit byte offsets from it, so a 16-byte load / store is
    // addressed as SGPR base + VGPR offset (no 64-bit VALU address per access); rows past M
    // read row M - 1, which is never below the base.  (m - b0) < 128, ldc < 2^24 (checked at
    // launch).
    [[maybe_unused]] const int64_t b0 = mrow < M ? mrow : M - 1;
    [[maybe_unused]] char* const ob = (char*)((_Float16*)ea.out + b0 * ea.ldc);
    [[maybe_unused]] auto obo = [&](int64_t m, int c) -> uint32_t {
        return (uint32_t)((int)(m - b0) * (int)ea.ldc + c) * 2u;
    };
    if (!BIAS_DONE && EPI != EPI_PATCH && ea.bias != nullptr) {
        float4 b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) b[j] = *(const float4*)(ea.bias + ncol + j * 16 + cq);
#pragma unroll
        for (int i = 0; i < NI; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                acc[i][j][0] += b[j].x;
                acc[i][j][1] += b[j].y;
                acc[i][j][2] += b[j].z;
                acc[i][j][3] += b[j].w;
            }
    }
    if constexpr (EPI == EPI_RESID_F16) {
        // Pair the fp32 accumulators first (v_permlane16_swap, see the fp16 path below; swap
        // whole uint4 images — per-element f32x4 read-modify-write around the builtin was
        // mis-lowered by hipcc 7.2, duplicating element 0 into elements 1..3):
        // afterwards lane group q holds columns colp(jp) .. +7 of its row in acc[i][2jp]
        // (first 4) and acc[i][2jp+1] (next 4) -> 16-byte fp16 loads and stores.
        const int q = lane >> 4;
#pragma unroll
        for (int i = 0; i < NI; i++)
#pragma unroll
            for (int jp = 0; jp < 2; jp++) {
                const uint4 a = __builtin_bit_cast(uint4, acc[i][2 * jp]);
                const uint4 c = __builtin_bit_cast(uint4, acc[i][2 * jp + 1]);
                const auto s0 = __builtin_amdgcn_permlane16_swap(a.x, c.x, false, false);
                const auto s1 = __builtin_amdgcn_permlane16_swap(a.y, c.y, false, false);
                const auto s2 = __builtin_amdgcn_permlane16_swap(a.z, c.z, false, false);
                const auto s3 = __builtin_amdgcn_permlane16_swap(a.w, c.w, false, false);
                acc[i][2 * jp] = __builtin_bit_cast(f32x4, make_uint4(s0[0], s1[0], s2[0], s3[0]));
                acc[i][2 * jp + 1] = __builtin_bit_cast(f32x4, make_uint4(s0[1], s1[1], s2[1], s3[1]));
            }
        auto colp = [&](int jp) { return ncol + (2 * jp + (q & 1)) * 16 + (q >> 1) * 8; };
        // the whole residual block is loaded before the first store (NI row groups, 2*NI
        // 16-byte loads in flight per lane: +6 % on out_proj at K = 768 over batches of 2)
        constexpr int NB = NI;
        auto store_batch = [&](int i0) {
#pragma unroll
            for (int ii = 0; ii < NB; ii++) {
                const int64_t m = mrow + (i0 + ii) * 16 + (lane & 15);
                const bool live = m < M;
                f16x8 h[2];
#pragma unroll
                for (int jp = 0; jp < 2; jp++) {
                    const f32x4 a = acc[i0 + ii][2 * jp], b = acc[i0 + ii][2 * jp + 1];
                    h[jp] = f16x8{(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3],
                                  (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
                    if constexpr (GEMM_VAR_NOSTORE) asm volatile("" ::"v"(h[jp]));
                    else if (live) *(f16x8*)(ob + obo(m, colp(jp))) = h[jp];
                }
                if (!GEMM_VAR_NOPSTAT && ea.pstat) {
                    // LayerNorm partials of the new fp16 row values over this wave's 64 columns
                    // (the 4 lane groups hold 16 each): sum, then the centred sum of squares
                    f32x2v sp = {0.f, 0.f};
#pragma unroll
                    for (int jp = 0; jp < 2; jp++)
#pragma unroll
                        for (int e = 0; e < 8; e += 2) sp += f32x2v{(float)h[jp][e], (float)h[jp][e + 1]};
                    float sum = sp.x + sp.y;
                    sum = xor16_sum(sum);
                    sum = xor32_sum(sum);
                    const f32x2v mu = {sum * (1.0f / 64), sum * (1.0f / 64)};
                    f32x2v dp = {0.f, 0.f};
#pragma unroll
                    for (int jp = 0; jp < 2; jp++)
#pragma unroll
                        for (int e = 0; e < 8; e += 2) {
                            const f32x2v d = f32x2v{(float)h[jp][e], (float)h[jp][e + 1]} - mu;
                            dp = __builtin_elementwise_fma(d, d, dp);
                        }
                    float m2 = dp.x + dp.y;
                    m2 = xor16_sum(m2);
                    m2 = xor32_sum(m2);
                    if (live && (lane >> 4) == 0) ea.pstat[(ncol >> 6) * ea.ldp + m] = make_float2(sum, m2);
                }
            }
        };
#pragma unroll
        for (int i0 = 0; i0 < NI; i0 += NB) {
            f16x8 xv[NB][2];
#pragma unroll
            for (int ii = 0; ii < NB; ii++) {
                int64_t m = mrow + (i0 + ii) * 16 + (lane & 15);
                m = m < M ? m : M - 1;  // clamped rows are loaded but not stored
#pragma unroll
                for (int jp = 0; jp < 2; jp++) {
                    if constexpr (GEMM_VAR_NORESLOAD) {  // timing variant: no residual read
                        xv[ii][jp] = f16x8{};
                        asm volatile("" : "+v"(xv[ii][jp]));
                    } else if constexpr (PRE) {
                        xv[ii][jp] = xpre[i0 + ii][jp];
                    } else {
                        xv[ii][jp] = *(const f16x8*)(ob + obo(m, colp(jp)));
                    }
                }
            }
            if (i0 > 0) store_batch(i0 - NB);
#pragma unroll
            for (int ii = 0; ii < NB; ii++)
#pragma unroll
                for (int jp = 0; jp < 2; jp++)
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        acc[i0 + ii][2 * jp][e] += (float)xv[ii][jp][e];
                        acc[i0 + ii][2 * jp + 1][e] += (float)xv[ii][jp][4 + e];
                    }
        }
        store_batch(NI - NB);
        return;
    }
    if constexpr (EPI == EPI_PATCH) {
        // software-pipelined: the loads of batch n+1 are issued before the stores of batch n,
        // so no wait ever covers a store (vmcnt retires in issue order).
        constexpr int NB = 2;  // row groups per batch: 8 float4 loads in flight per lane
        auto row_of = [&](int i) {
            const int64_t m = mrow + i * 16 + (lane & 15);
            return m < M ? m : M - 1;  // clamped rows are loaded but not stored
        };
        auto src_row = [&](int64_t m) -> const float* {
            return ea.pos + (1 + (uint32_t)m % (uint32_t)ea.npatch) * (int64_t)N + ncol + cq;
        };
        auto store_batch = [&](int i0) {
            const int q = lane >> 4;
#pragma unroll
            for (int ii = 0; ii < NB; ii++) {
                const int64_t m = mrow + (i0 + ii) * 16 + (lane & 15);
                // patch rows of the fp16 residual stream; 16-byte stores after the fp16 path's
                // v_permlane16_swap pairing (lane group q: 8 columns of fragment 2jp + (q & 1))
                const uint32_t mc = (uint32_t)(m < M ? m : M - 1);
                const uint32_t img = mc / (uint32_t)ea.npatch, p = mc - img * (uint32_t)ea.npatch;
                _Float16* d = (_Float16*)ea.out + ((int64_t)img * ea.seq + 1 + p) * ea.ldc + ncol;
#pragma unroll
                for (int jp = 0; jp < 2; jp++) {
                    const f32x4 a = acc[i0 + ii][2 * jp], c = acc[i0 + ii][2 * jp + 1];
                    const auto lo = __builtin_amdgcn_permlane16_swap(cvt_pk_f16(a[0], a[1]), cvt_pk_f16(c[0], c[1]),
                                                                     false, false);
                    const auto hi = __builtin_amdgcn_permlane16_swap(cvt_pk_f16(a[2], a[3]), cvt_pk_f16(c[2], c[3]),
                                                                     false, false);
                    if (m < M)
                        *(uint4*)(d + (2 * jp + (q & 1)) * 16 + (q >> 1) * 8) = make_uint4(lo[0], hi[0], lo[1], hi[1]);
                }
            }
        };
#pragma unroll
        for (int i0 = 0; i0 < NI; i0 += NB) {
            float4 x[NB][4];
#pragma unroll
            for (int ii = 0; ii < NB; ii++) {
                const float* sp = src_row(row_of(i0 + ii));
#pragma unroll
                for (int j = 0; j < 4; j++) x[ii][j] = *(const float4*)(sp + j * 16);
            }
            if (i0 > 0) store_batch(i0 - NB);
#pragma unroll
            for (int ii = 0; ii < NB; ii++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    acc[i0 + ii][j][0] += x[ii][j].x;
                    acc[i0 + ii][j][1] += x[ii][j].y;
                    acc[i0 + ii][j][2] += x[ii][j].z;
                    acc[i0 + ii][j][3] += x[ii][j].w;
                }
        }
        store_batch(NI - NB);
        return;
    }
    if constexpr (EPI == EPI_RRHI) {
        // the items' norms: columns (4 consecutive per lane and fragment) and rows
        const int64_t n = ea.rr_n;
        const float* csq = ea.rr_csqn ? ea.rr_csqn : ea.rr_sqn;
        const float* cnr = ea.rr_cnrm ? ea.rr_cnrm : ea.rr_nrm;
        float sj[4][4], nj[4][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t c0 = ncol + j * 16 + cq;
            if (c0 + 3 < n) {
                const float4 a = *(const float4*)(csq + c0), b = *(const float4*)(cnr + c0);
                sj[j][0] = a.x, sj[j][1] = a.y, sj[j][2] = a.z, sj[j][3] = a.w;
                nj[j][0] = b.x, nj[j][1] = b.y, nj[j][2] = b.z, nj[j][3] = b.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int64_t c = c0 + e < n ? c0 + e : n - 1;
                    sj[j][e] = csq[c];
                    nj[j][e] = cnr[c];
                }
            }
        }
        float si[NI], ni[NI];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int64_t m = mrow + i * 16 + (lane & 15);
            const int64_t g = ea.rr_row0 + (m < M ? m : M - 1);
            si[i] = ea.rr_sqn[g];
            ni[i] = ea.rr_nrm[g];
        }
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int64_t m = mrow + i * 16 + (lane & 15);
            if (m >= M) continue;
            const float crn = ea.rr_c[0] * ni[i];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int64_t c0 = ncol + j * 16 + cq;
                float h[4];
#pragma unroll
                for (int e = 0; e < 4; e++)
                    h[e] = c0 + e < n ? rr_hi(acc[i][j][e], si[i], sj[j][e], crn, ni[i], nj[j][e], ea.rr_c)
                                      : __builtin_inff();
                *(float4*)((float*)ea.out + m * ea.ldc + c0) = make_float4(h[0], h[1], h[2], h[3]);
            }
        }
        return;
    }
    if constexpr (EPI == EPI_F32) {
        if (ea.dist_rsq != nullptr) {  // Euclidean distance: the same fp32 operations as a separate pass
            const int64_t n = ea.dist_n;
            float sj[4][4];
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int64_t c = ncol + j * 16 + cq + e;
                    sj[j][e] = ea.dist_csq[c < n ? c : n - 1];
                }
            const bool vec = (ea.ldc & 3) == 0 && ((uintptr_t)ea.out & 15) == 0;
#pragma unroll
            for (int i = 0; i < NI; i++) {
                const int64_t m = mrow + i * 16 + (lane & 15);
                if (m >= M) continue;
                const float si = ea.dist_rsq[m];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int64_t c0 = ncol + j * 16 + cq;
                    float h[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) h[e] = (si + sj[j][e]) - 2.0f * acc[i][j][e];
                    float* o = (float*)ea.out + m * ea.ldc + c0;
                    if (vec && c0 + 3 < n) {
                        *(float4*)o = make_float4(h[0], h[1], h[2], h[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            if (c0 + e < n) o[e] = h[e];
                    }
                }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int64_t m = mrow + i * 16 + (lane & 15);
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const f32x4 v = acc[i][j];
                *(float4*)((float*)ea.out + m * ea.ldc + ncol + j * 16 + cq) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
        return;
    }
    // fp16 outputs.  v^T tiles of the head split keep the scattered 2-byte stores.
    // Head split: the wave's 64 columns lie inside one of q / k / v (wd is a multiple of 64),
    // so the q/k/v selector and the column's offset inside it are wave-uniform; the token
    // index (b, t) of a row comes from one 32-bit division per row group (M < 2^31, checked
    // at launch) instead of 64-bit divisions per fragment.
    [[maybe_unused]] int qkv_sel = 0, qkv_c0 = 0;
    if constexpr (EPI == EPI_QKV) {
        const int wd = ea.heads * 64;
        const int nb = __builtin_amdgcn_readfirstlane(ncol + ea.n_off);
        qkv_sel = nb / wd;
        qkv_c0 = nb - qkv_sel * wd;
        if (qkv_sel == 2) {
            const uint32_t seq = (uint32_t)ea.seq;
            const int64_t lp = ea.lpad;
#pragma unroll
            for (int i = 0; i < NI; i++) {
                const int64_t m = mrow + i * 16 + (lane & 15);
                if (m >= M) continue;
                const uint32_t b = (uint32_t)m / seq, t = (uint32_t)m - b * seq;
                _Float16* vb = (_Float16*)ea.vt + (int64_t)b * ea.heads * 64 * lp + t;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const f32x4 v = acc[i][j];
                    const int hd = qkv_c0 + j * 16 + cq;  // h * 64 + d
                    _Float16* dst = vb + (int64_t)hd * lp;
                    dst[0] = (_Float16)v[0];
                    dst[lp] = (_Float16)v[1];
                    dst[2 * lp] = (_Float16)v[2];
                    dst[3 * lp] = (_Float16)v[3];
                }
            }
            return;
        }
    }
    // Row-per-lane store widening (cdna_hip_programming.md T21, 16-lane form): lane group
    // q = lane>>4 holds columns 4q..4q+3 of fragments j and j+1; one v_permlane16_swap per
    // packed dword leaves groups 0/2 with 8 consecutive columns of fragment j and groups
    // 1/3 with 8 of fragment j+1 -> one 16-byte store per lane per fragment pair.
    const int q = lane >> 4;
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int64_t m = mrow + i * 16 + (lane & 15);
        [[maybe_unused]] _Float16* qkrow = nullptr;  // QKV: q / k row (b, h = 0, t)
        if constexpr (EPI == EPI_QKV) {
            const uint32_t seq = (uint32_t)ea.seq;
            const uint32_t b = (uint32_t)m / seq, t = (uint32_t)m - b * seq;
            qkrow = (_Float16*)(qkv_sel == 0 ? ea.q : ea.k) + ((int64_t)b * ea.heads * ea.seq + t) * 64;
        }
#pragma unroll
        for (int jp = 0; jp < 2; jp++) {
            f32x4 a = acc[i][2 * jp], c = acc[i][2 * jp + 1];
            if constexpr (EPI == EPI_GELU_H16 && !GEMM_VAR_NOGELU) {
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const f32x2v ga = quick_gelu2(f32x2v{a[e], a[e + 1]});
                    const f32x2v gc = quick_gelu2(f32x2v{c[e], c[e + 1]});
                    a[e] = ga.x;
                    a[e + 1] = ga.y;
                    c[e] = gc.x;
                    c[e + 1] = gc.y;
                }
            }
            const auto lo = __builtin_amdgcn_permlane16_swap(cvt_pk_f16(a[0], a[1]), cvt_pk_f16(c[0], c[1]), false, false);
            const auto hi = __builtin_amdgcn_permlane16_swap(cvt_pk_f16(a[2], a[3]), cvt_pk_f16(c[2], c[3]), false, false);
            const uint4 v = make_uint4(lo[0], hi[0], lo[1], hi[1]);
            const int col = ncol + (2 * jp + (q & 1)) * 16 + (q >> 1) * 8;
            if (!FULL && m >= M) continue;
            if constexpr (EPI == EPI_QKV) {
                const int hd = qkv_c0 + (col - ncol);  // h * 64 + d
                *(uint4*)(qkrow + (int64_t)(hd >> 6) * ea.seq * 64 + (hd & 63)) = v;
            } else {
                if constexpr (GEMM_VAR_NOSTORE) {  // timing variant: value kept, no store
                    typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
                    asm volatile("" ::"v"(__builtin_bit_cast(u32x4v, v)));
                }
                else *(uint4*)(ob + obo(m, col)) = v;
            }
        }
    }
}

template <int EPI>
struct EpiVm {  // vector-memory instructions of one full-tile epilogue_tile<EPI, 8> per wave
                // (EPI_RRHI: its 32 stores; its norm loads complete before the first store)
    static constexpr int count = EPI == EPI_H16 || EPI == EPI_GELU_H16 || EPI == EPI_QKV ? 16
                                 : EPI == EPI_RESID_F16 || EPI == EPI_F32 || EPI == EPI_RRHI ? 32
                                                                                          : -1;
};

}  // namespace reidmi
