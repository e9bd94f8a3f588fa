// gemm.hip — fp16 MFMA GEMM (C = A . W^T) with fused epilogues; see gemm.h.
//
// Every operand is fp16 (the reference's GPU dtype, utils.py:145-166), fp32 accumulation on
// v_mfma_f32_16x16x32_f16.  Two tilings, bit-identical per output element (same MFMA chain,
// K ascending):
//  * gemm_tile_kernel (small M: the CLS-only last block, proj, the text tower's heads):
//    128x128x64 block tile, 256 threads = 4 waves as 2x2, each wave 64x64 = 4x4 MFMA tiles;
//    operands staged global -> registers -> LDS (double-buffered, one barrier per K-step).
//  * gemm_persistent_kernel (>= 256 tiles of 256x256): see its header below.
// LDS rows are 128 B; 16-byte chunks are XOR-swizzled with (row>>1)&7 so the fragment
// reads (16 rows x 4 chunks per ds_read_b128 lane group) are bank-conflict free.  Operands
// are swapped in the MFMA (W fragment as A, activation fragment as B) so each lane ends up
// holding one output row and 4 consecutive output columns: epilogue loads/stores are 8-16 B
// per lane.
#include "gemm.h"
#include <type_traits>

#include <mutex>
#include <vector>

namespace reidmi {

// ----------------------------------------------------------- live GEMM timing
// bench.py measures the roofline of the dominant kernel with HIP events recorded on the
// launch stream around each GEMM of the timed region (reidmi_prof_*).  Off by default.
namespace prof {
struct Rec {
    hipEvent_t a, b;
    double flops;
    int epi;
};
static bool enabled = false;
static std::mutex mu;
static std::vector<Rec> recs;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
static size_t used = 0;
}  // namespace prof

constexpr int GB_M = 128, GB_N = 128, GB_K = 64;

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
__global__ __launch_bounds__(256, 2) void gemm_tile_kernel(const _Float16* __restrict__ A, int64_t lda,
                                                           const _Float16* __restrict__ W, int64_t ldw, int64_t M,
                                                           int N, int K, EpiArgs ea, int tiles_n, int nwg) {
    __shared__ __attribute__((aligned(16))) _Float16 smem[2][2][GB_M * GB_K];
    const int bid = blockIdx.x;
    const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
    const int wg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
    const int tm = wg / tiles_n, tn = wg % tiles_n;
    const int64_t m0 = (int64_t)tm * GB_M;
    const int n0 = tn * GB_N;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;

    // per-thread staging slots: 4 x 16 B of A and of W per K-step
    const _Float16* gA[4];
    const _Float16* gW[4];
    int soff[4];
    bool aval[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int c = tid + 256 * u, row = c >> 3, kc = c & 7;
        aval[u] = m0 + row < M;
        gA[u] = A + (aval[u] ? (m0 + row) : 0) * lda + kc * 8;
        gW[u] = W + (int64_t)(n0 + row) * ldw + kc * 8;
        soff[u] = swz(row, kc);
    }
    uint4 ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3;
#define GLOAD(k0)                                                                  \
    do {                                                                           \
        ra0 = aval[0] ? *(const uint4*)(gA[0] + (k0)) : make_uint4(0, 0, 0, 0);   \
        ra1 = aval[1] ? *(const uint4*)(gA[1] + (k0)) : make_uint4(0, 0, 0, 0);   \
        ra2 = aval[2] ? *(const uint4*)(gA[2] + (k0)) : make_uint4(0, 0, 0, 0);   \
        ra3 = aval[3] ? *(const uint4*)(gA[3] + (k0)) : make_uint4(0, 0, 0, 0);   \
        rw0 = *(const uint4*)(gW[0] + (k0));                                       \
        rw1 = *(const uint4*)(gW[1] + (k0));                                       \
        rw2 = *(const uint4*)(gW[2] + (k0));                                       \
        rw3 = *(const uint4*)(gW[3] + (k0));                                       \
    } while (0)
#define LSTORE(buf)                                                                \
    do {                                                                           \
        *(uint4*)(&smem[buf][0][soff[0]]) = ra0;                                   \
        *(uint4*)(&smem[buf][0][soff[1]]) = ra1;                                   \
        *(uint4*)(&smem[buf][0][soff[2]]) = ra2;                                   \
        *(uint4*)(&smem[buf][0][soff[3]]) = ra3;                                   \
        *(uint4*)(&smem[buf][1][soff[0]]) = rw0;                                   \
        *(uint4*)(&smem[buf][1][soff[1]]) = rw1;                                   \
        *(uint4*)(&smem[buf][1][soff[2]]) = rw2;                                   \
        *(uint4*)(&smem[buf][1][soff[3]]) = rw3;                                   \
    } while (0)

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    GLOAD(0);
    LSTORE(0);
    __syncthreads();
    const int nk = K / GB_K;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) GLOAD((kt + 1) * GB_K);
        const _Float16* sA = smem[cur][0];
        const _Float16* sW = smem[cur][1];
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            f16x8 af[4], wf[4];
            const int kc = ks * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < 4; i++) af[i] = *(const f16x8*)(sA + swz(wm * 64 + i * 16 + (lane & 15), kc));
#pragma unroll
            for (int j = 0; j < 4; j++) wf[j] = *(const f16x8*)(sW + swz(wn * 64 + j * 16 + (lane & 15), kc));
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = mfma16(wf[j], af[i], acc[i][j]);
        }
        if (kt + 1 < nk) LSTORE(cur ^ 1);
        __syncthreads();
    }

    // ------------------------------------------------------------------ epilogue
    if (ea.rowstat) {
        float4 bn[4];
        const int cq = (lane >> 4) * 4;
#pragma unroll
        for (int j = 0; j < 4; j++)
            bn[j] = ea.bias ? *(const float4*)(ea.bias + n0 + wn * 64 + j * 16 + cq) : make_float4(0.f, 0.f, 0.f, 0.f);
        ln_fold<4>(acc, ea.rowstat, ea.colsum, bn, m0 + wm * 64, n0 + wn * 64, M);
        epilogue_tile<EPI, 4, true>(ea, acc, m0 + wm * 64, n0 + wn * 64, M, N);
        return;
    }
    epilogue_tile<EPI, 4>(ea, acc, m0 + wm * 64, n0 + wn * 64, M, N);
#undef GLOAD
#undef LSTORE
}

// ================================================================ persistent tile
// 256x256x64 block tile, 512 threads = 8 waves as 2 (M) x 4 (N), 128x64 per wave (8x4 tiles
// of 16x16x32): half the LDS bytes per FLOP of the 64x64-per-wave 128x128 tile.  Operands go
// HBM -> LDS by global_load_lds_dwordx4 (no VGPR staging): one wave-instruction fills 1 KiB =
// 8 LDS rows of 128 B, lane l -> row 8j + l/8, physical 16-B chunk l%8.  The (row>>1)&7 XOR
// swizzle is applied on the per-lane SOURCE address (logical chunk kc = physical ^ swz(row)),
// and the same XOR on the ds_read side, so LDS stays lane-linear and fragment reads stay
// conflict-free.  All LDS is one dynamic array (a second __shared__ object makes hipcc drain
// vmcnt before every ds_read).
constexpr int G2_M = 256, G2_N = 256;
constexpr int G2_STAGE = (G2_M + G2_N) * GB_K;  // fp16 elements per stage

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// Schedule (per K-step of 64): 4 LOAD sections (ds_read of the fragments of one 64x32
// output quadrant, issue a share of the DMA for a later K-step, lgkmcnt(0)) interleaved with
// 4 COMPUTE sections (16 register-only MFMAs), one raw s_barrier after each section.  Waves
// 4-7 run one barrier behind waves 0-3, so on every SIMD (waves w and w+4) one wave reads LDS
// while the other multiplies.  Quadrant order (0,0),(0,1),(1,1),(1,0) reuses A or W
// fragments between sections.  Region DMA: each operand stage is 4 regions of 128 LDS rows
// (16 pieces of 8 rows): A0 = rows {0..63, 128..191} (quadrant 0 of both wave rows), A1 =
// the other 128; B0 = W rows {wc*64 + 0..31}, B1 = W rows {wc*64 + 32..63}; wave w moves
// pieces 2w, 2w+1 of a region.  A region is refilled for K-step s+2 right after its last read
// in K-step s, so the only wait is one counted vmcnt(6) per K-step.
//
// Persistent: grid = min(#tiles, 256) (one workgroup per CU).  The two DMA streams — "+1"
// (region B0 of the next K-step) and "+2" (A0, B1, A1 of the K-step after) — run over the
// workgroup's concatenated (tile, K-step) sequence, so while a tile's epilogue runs, the next
// tile's first two K-steps are already landing.  Both groups run the epilogue in one barrier
// slot (their store tails overlap: +1 % c_fc, +2-6 % out_proj over running them back to
// back, profiles/r02/gemm_epilogue_sync_ab.txt).
//
// Tile walk (XCD-aware): workgroup b runs on XCD b % 8.  The XCDs are split into `ngroups`
// groups; group k owns the N-tiles [k T_n / ngroups, (k+1) T_n / ngroups), and each XCD of
// the group owns a contiguous range of that group's (M-tile, N-tile) sequence (M-major), its
// 32 workgroups striding through it — so the tiles an XCD runs at once share A row panels in
// its L2, and with ngroups > 1 the W panels an XCD re-reads shrink to its N share.
//
// Deferred epilogue stores: the epilogue's stores are not waited for by the next tile's first
// K-step.  vmcnt retires in issue order, so a plain `vmcnt(6)` after an epilogue would wait
// for every store the epilogue issued (one HBM write round trip per tile, MFMAs idle).  The
// next tile's first "+1" DMA (B0 of its K-step 1) is issued BEFORE the epilogue, and that
// step's wait counts the epilogue's memory instructions as allowed to be outstanding:
// vmcnt(6 + S (+ the tile's bias / colsum / rowstat DMAs)), S = EpiVm<EPI>::count (global
// load/store instructions per wave and full tile, counted from the ISA; with LayerNorm
// partials the residual epilogue issues 8 more stores, so S is then a lower bound — safe,
// as vmcnt retires in order).  Only after a full tile (no masked rows) and not for
// scattered-v^T QKV tiles; otherwise the plain vmcnt(6).  The bias is read from LDS by
// inline ds_read (the compiler would insert a vmcnt(0) before a ds_read of an LDS-DMA'd
// slot, draining the in-flight DMA every tile).  All tilings run the same MFMA chain per
// output element -> bit-identical results.
// ---- EPI_RRSV (the R2 pre-filter's survivors, gemm.h) in the persistent kernel.  Per row
// group i and column group j a lane holds 4 pairs; their hi = rr_hi(acc) (packed fp32, the
// same roundings as rr_hi) is compared with the row's thresholds, and the survivors are
// appended to a per-wave buffer in LDS: 8-byte entries (tile sequence number << 13 | row in
// the wave's 128 << 6 | column in its 64, bit 31 = the pair as (column, row); hi bits), lane
// offsets from ballots.  The row and
// column records (norms, thresholds) arrive by LDS-DMA at the tile's first K-step, into one
// of two buffers by tile parity (a wave still reading tile t's records cannot be overtaken by
// tile t+2's DMA: every wave passes tile t+1's barriers in between).  So the epilogue issues
// no global memory instruction; a flush (one atomic add per entry on the row's counter, the
// pair stored at the returned position) runs when the next (i, j) group could overflow the
// buffer and once after the workgroup's last tile: typical tiles hold ~10 survivors per wave,
// so the atomic round trip is paid every few dozen tiles, not per tile.
// LDS, after the two operand stages: row records [2][256] float4 (8 KiB), column records
// [2][256] float4 (8 KiB), survivor buffers [8 waves][kRrsvWaveCap] int2 (16 KiB).
// A group's tile sequence t -> (M-tile, N-tile within the group): band = 0, M-major (t / tnk,
// t % tnk); band > 0, bands of `band` M-tiles walked N-major, so the tiles one XCD runs at
// once form a band x (32 / band) block and share both operands' panels in its L2 (the
// re-rank's N x N products, where neither operand fits a cache; gemm_f16).
template <bool LIST = false>
__device__ __forceinline__ void tile_mn(int t, int tnk, int band, int tiles_m, const int* list, int& mt, int& nt) {
    if constexpr (LIST) {  // EPI_RRSV's tile list (gemm.h rr_tiles)
        // constant address space: a scalar load (lgkmcnt), not a vector load whose wait would
        // drain the operand DMA in flight
        const int v = ((const __attribute__((address_space(4))) int*)list)[t];
        mt = v >> 16;
        nt = v & 0xffff;
        return;
    }
    if (band <= 0) {
        mt = t / tnk;
        nt = t - mt * tnk;
        return;
    }
    const int per = band * tnk, b = t / per, r = t - b * per;
    const int rows = tiles_m - b * band < band ? tiles_m - b * band : band;
    nt = r / rows;
    mt = b * band + (r - nt * rows);
}

#ifndef RR_GEMM_BAND
#define RR_GEMM_BAND 8
#endif
constexpr int kRrsvWaveCap = 256;  // >= one (i, j) group: 16 rows x 16 columns
constexpr int kRrsvSlotBytes = 8192 + 8192 + 8 * kRrsvWaveCap * 8;
struct RrsvWalk {
    int first, gx, wr, wc;  // the persistent walk (tile = first + seq * gx) over the tile list
    const int* list;
};

__device__ __forceinline__ void rrsv_flush(const EpiArgs& ea, uint32_t sv_lds, int& sv_n, int lane,
                                           const RrsvWalk& w) {
    for (int t0 = 0; t0 < sv_n; t0 += 64) {
        const int t = t0 + lane;
        int2 e;
        // inline ds_read: the compiler would wait for the operand DMA in flight (vmcnt(0))
        // before a plain LDS read
        asm volatile("ds_read_b64 %0, %1" : "=v"(e) : "v"(sv_lds + 8u * (uint32_t)(t < sv_n ? t : 0)) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e)::"memory");
        if (t < sv_n) {
            int mt, nt;
            tile_mn<true>(w.first + (int)(((uint32_t)e.x >> 13) & 0x3ffff) * w.gx, 1, 0, 0, w.list, mt, nt);
            const int64_t mi = (int64_t)mt * 256 + w.wr * 128 + ((e.x >> 6) & 127);
            const int ci = nt * 256 + w.wc * 64 + (e.x & 63);
            const bool tr = e.x < 0;  // bit 31: the pair belongs to the column item's row
            const int64_t m = tr ? ci : mi;
            const int col = tr ? (int)mi : ci;
            const int p = atomicAdd(ea.sv_cnt + m, 1);
            if (p < ea.sv_cap) ea.sv_list[m * ea.sv_cap + p] = make_int2(col, e.y);
        }
    }
    sv_n = 0;
}

// rows_lds / cols_lds: LDS byte addresses of this tile's record buffers (parity applied);
// both: the tile is above the diagonal of a symmetric product (rr_tri), so each pair is also
// tested as (column, row)
__device__ __forceinline__ void rrsv_tile(const EpiArgs& ea, const f32x4 (&acc)[8][4], int64_t mrow, int ncol,
                                          int64_t M, int seq, bool both, uint32_t rows_lds, uint32_t cols_lds,
                                          uint32_t sv_lds, int& sv_n, int lane, const RrsvWalk& w) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    const int64_t n = ea.rr_n;
    const int cq = (lane >> 4) * 4;
    const uint64_t below = (1ull << lane) - 1;
    // appends the lane's pairs e with bit e of b: the group's total and the lanes' offsets
    // from ballots (counts 0..4), a flush first when the buffer could overflow
    auto append = [&](uint32_t b, int key, f32x4 h) {
        const uint64_t v1 = __builtin_amdgcn_ballot_w64(b != 0);
        if (v1 == 0) return;
        const int c = __builtin_popcount(b);
        const uint64_t v2 = __builtin_amdgcn_ballot_w64(c > 1), v3 = __builtin_amdgcn_ballot_w64(c > 2),
                       v4 = __builtin_amdgcn_ballot_w64(c > 3);
        const int tot = __builtin_popcountll(v1) + __builtin_popcountll(v2) + __builtin_popcountll(v3) +
                        __builtin_popcountll(v4);
        if (sv_n + tot > kRrsvWaveCap) rrsv_flush(ea, sv_lds, sv_n, lane, w);  // tot <= 256
        int p = sv_n + __builtin_popcountll(v1 & below) + __builtin_popcountll(v2 & below) +
                __builtin_popcountll(v3 & below) + __builtin_popcountll(v4 & below);
        // the whole vector reinterpreted at once: a bit_cast of one element of a float vector
        // read element 0 (hipcc 7.2)
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        const i32x4 hb = __builtin_bit_cast(i32x4, h);
#pragma unroll
        for (int e = 0; e < 4; e++)
            if ((b >> e) & 1u) {
                const int2 ent = make_int2(key + e, hb[e]);
                asm volatile("ds_write_b64 %0, %1" ::"v"(sv_lds + 8u * (uint32_t)p), "v"(ent) : "memory");
                p++;
            }
        sv_n += tot;
    };
    const uint32_t ca = cols_lds + 16u * (uint32_t)(w.wc * 64 + cq);
    const uint32_t ra = rows_lds + 16u * (uint32_t)(w.wr * 128 + (lane & 15));
    // one sweep over the lane's pairs; TR: as (column, row) against the column item's
    // thresholds.  Two separate loop nests (one sweep each): a single nest with both appends
    // is too large to unroll, and the accumulators would go to scratch.
    auto sweep = [&](auto tr_c) {
        constexpr bool TR = decltype(tr_c)::value;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // columns cq + 16 j + e: (s_c, n_c, hi_max_c, lb_c)
            f32x4 cr[4];
            const uint32_t caj = ca + 256u * j;
            asm volatile("ds_read_b128 %0, %1" : "=v"(cr[0]) : "v"(caj) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(cr[1]) : "v"(caj) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(cr[2]) : "v"(caj) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:48" : "=v"(cr[3]) : "v"(caj) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cr[0]), "+v"(cr[1]), "+v"(cr[2]), "+v"(cr[3])::"memory");
            const f2 sj0 = {cr[0][0], cr[1][0]}, sj1 = {cr[2][0], cr[3][0]};
            const f2 nj0 = {cr[0][1], cr[1][1]}, nj1 = {cr[2][1], cr[3][1]};
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int64_t m = mrow + i * 16 + (lane & 15);
                f32x4 rm;  // (s_m, n_m, hi_max, lb)
                asm volatile("ds_read_b128 %0, %1" : "=v"(rm) : "v"(ra + 256u * i) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rm)::"memory");
                const f2 si = {rm[0], rm[0]}, ni = {rm[1], rm[1]};
                // hi of the pairs: rr_hi's operations on two lanes of packed fp32; as (column,
                // row) it is rr_hi with the roles swapped (the product term c_rel n_c . n_m)
                auto hi2 = [&](f2 sj, f2 nj, f2 dot) -> f2 {
                    const f2 sum = si + sj;
                    const f2 dt = __builtin_elementwise_fma(f2{-2.0f, -2.0f}, dot, sum);
                    return TR ? dt + 1.01f * (__builtin_elementwise_fma(ea.rr_c[0] * nj, ni, 0x1p-23f * sum) +
                                              ea.rr_c[1] * (nj + ni) + ea.rr_c[2])
                              : dt + 1.01f * (__builtin_elementwise_fma(ea.rr_c[0] * ni, nj, 0x1p-23f * sum) +
                                              ea.rr_c[1] * (ni + nj) + ea.rr_c[2]);
                };
                const f2 h01 = hi2(sj0, nj0, f2{acc[i][j][0], acc[i][j][1]});
                const f2 h23 = hi2(sj1, nj1, f2{acc[i][j][2], acc[i][j][3]});
                const f32x4 h = {h01.x, h01.y, h23.x, h23.y};
                // a pair survives unless lb < hi < hi_max, so a NaN or infinite bound survives
                // too and sends the row to the exact path (rank_select_sv)
                uint32_t b = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float hx = TR ? cr[e][2] : rm[2], lb = TR ? cr[e][3] : rm[3];
                    b |= (uint32_t)(m < M && ncol + j * 16 + cq + e < n && !(h[e] > hx && h[e] < lb)) << e;
                }
                const int key = (seq << 13) | ((i * 16 + (lane & 15)) << 6) | (j * 16 + cq);
                append(b, TR ? key | (int)0x80000000u : key, h);
            }
        }
    };
    sweep(std::false_type{});
    if (both) sweep(std::true_type{});
}

template <int EPI>
struct EpiVm {  // vector-memory instructions of one full-tile epilogue_tile<EPI, 8> per wave
                // (EPI_RRHI: its 32 stores; its norm loads complete before the first store)
    static constexpr int count = EPI == EPI_H16 || EPI == EPI_GELU_H16 || EPI == EPI_QKV ? 16
                                 : EPI == EPI_RESID_F16 || EPI == EPI_F32 || EPI == EPI_RRHI ? 32
                                                                                          : -1;
};

// TAG: a symbol tag only (same code): the residual epilogue's two callers, out_proj (K = W,
// TAG 0) and mlp.c_proj (K = 4W, TAG 1), get their own kernel names in rocprof traces
template <int EPI, int TAG = 0>
__global__ __launch_bounds__(512, 2) void gemm_persistent_kernel(const _Float16* __restrict__ A, int64_t lda,
                                                                 const _Float16* __restrict__ W, int64_t ldw,
                                                                 int64_t M, int N, int K, EpiArgs ea, int tiles_m,
                                                                 int tiles_n, int ngroups, int band) {
    extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
    const int G = gridDim.x;
    const int bid = blockIdx.x;
    const int ng = G < 8 ? G : 8;
    const int xg = bid % ng, gx = G / ng + ((G % ng) > xg ? 1 : 0);
    const int ngr = (ng == 8 && 8 % ngroups == 0 && ngroups <= tiles_n) ? ngroups : 1;
    const int xper = ng / ngr, grp = xg / xper, xs = xg - grp * xper;
    const int nb0 = tiles_n * grp / ngr, tnk = tiles_n * (grp + 1) / ngr - nb0;  // this group's N-tiles
    const int64_t sub = (int64_t)tiles_m * tnk;
    const int lo = (int)(sub * xs / xper), hi = (int)(sub * (xs + 1) / xper);
    const int first = lo + bid / ng;
    if (first >= hi) return;
    if constexpr (EPI == EPI_RESID_F16) {
        // The residual epilogue reads and writes 2 x 128 KB per tile; with every workgroup in
        // step those bursts hit HBM together.  Odd workgroups start ~8k cycles (~1/8 of an
        // out_proj tile) late: out_proj -2.5 %, c_proj -1.7 %; no effect on the other epilogues
        // (profiles/r04/gemm_stagger_prefetch_ab.txt)
        if (bid & 1) __builtin_amdgcn_s_sleep(127);
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2, wc = wid & 3;
    const int nk = K / GB_K;

    // per-lane DMA geometry: piece pc = 2*wid + u of region half h
    int rowA[2][2], kcA[2][2], offA[2][2], offW[2][2];
    uint32_t offAb[2][2], offWb[2][2];  // byte offsets from the tile's (row 0, k0) element
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int pc = 2 * wid + u;
            const int ra = 128 * (pc >> 3) + 64 * h + 8 * (pc & 7);
            const int rb = 64 * (pc >> 2) + 32 * h + 8 * (pc & 3);
            const int r1 = ra + (lane >> 3), r2 = rb + (lane >> 3);
            rowA[h][u] = r1;
            kcA[h][u] = ((lane & 7) ^ ((r1 >> 1) & 7)) * 8;
            offAb[h][u] = (uint32_t)(r1 * (int)lda + kcA[h][u]) * 2u;
            offWb[h][u] = (uint32_t)(r2 * (int)ldw + ((lane & 7) ^ ((r2 >> 1) & 7)) * 8) * 2u;
            offA[h][u] = ra * GB_K;
            offW[h][u] = G2_M * GB_K + rb * GB_K;
        }
    const int* const rr_list = EPI == EPI_RRSV ? ea.rr_tiles : nullptr;  // (gemm.h rr_tiles)
    if constexpr (EPI != EPI_RRHI) band = 0;  // bands: the re-rank's dense product only
    // a DMA stream position: tile (m0, n0), K-step, and whether all 256 A rows exist
    // a: byte address of A[m0][kt * GB_K], w: of W[n0][kt * GB_K] -- computed once per tile
    // and stepped by one K-step's bytes, so a DMA issue costs no 64-bit multiply (scalar
    // instructions of the LOAD phases, which run beside the partner wave's MFMAs)
    struct Pos {
        int tile, kt;
        int64_t m0;
        int n0;
        bool full;
        const char* a;
        const char* w;
    };
    auto set_tile = [&](Pos& p, int tile) {
        p.tile = tile;
        p.kt = 0;
        int mt, nt;
        tile_mn<EPI == EPI_RRSV>(tile, tnk, band, tiles_m, rr_list, mt, nt);
        p.m0 = (int64_t)mt * G2_M;
        p.n0 = (nb0 + nt) * G2_N;
        p.full = p.m0 + G2_M <= M;
        p.a = (const char*)(A + (GEMM_VAR_ASAME ? 0 : p.m0) * lda);
        p.w = (const char*)(W + (int64_t)p.n0 * ldw);
    };
    auto advance = [&](Pos& p) {
        if (++p.kt == nk) {
            set_tile(p, p.tile + gx);
        } else {
            p.a += GB_K * 2;
            p.w += GB_K * 2;
        }
    };
    // uniform tile base + per-lane 32-bit byte offset (SGPR base + VGPR offset form)
    auto issue_a = [&](int stage, int h, const Pos& p) {
        const char* base = p.a;
        if (p.full) {
#pragma unroll
            for (int u = 0; u < 2; u++)
                __builtin_amdgcn_global_load_lds(base + offAb[h][u],
                                                 (lds_ptr_t)(lds + stage * G2_STAGE + offA[h][u]), 16, 0, 0);
        } else {  // partial last row tile: rows >= M read row M-1 (never stored)
            const int lim = (int)(M - p.m0);
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int r = rowA[h][u] < lim ? rowA[h][u] : lim - 1;
                __builtin_amdgcn_global_load_lds(base + (uint32_t)(r * (int)lda + kcA[h][u]) * 2u,
                                                 (lds_ptr_t)(lds + stage * G2_STAGE + offA[h][u]), 16, 0, 0);
            }
        }
    };
    auto issue_w = [&](int stage, int h, const Pos& p) {
        const char* base = p.w;
#pragma unroll
        for (int u = 0; u < 2; u++)
            __builtin_amdgcn_global_load_lds(base + offWb[h][u],
                                             (lds_ptr_t)(lds + stage * G2_STAGE + offW[h][u]), 16, 0, 0);
    };
#define G5_BARRIER()                              \
    do {                                          \
        __builtin_amdgcn_sched_barrier(0);        \
        __builtin_amdgcn_s_barrier();             \
        __builtin_amdgcn_sched_barrier(0);        \
    } while (0)
#define G5_LDS_DONE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

    // Both column halves' W fragments stay in registers (6 more VGPRs as allocated), so
    // LOAD 3 reads nothing: the K-step's W fragments are read from LDS once, not 1.5 times
    // (-14 % LDS read bytes; c_fc / QKV / c_proj +1 %, out_proj even,
    // profiles/r04/gemm_fb2_ab.txt)
    f16x8 fa[4][2], fbq[2][2][2];
    f32x4 acc[8][4];
    auto load_a = [&](const _Float16* sA, int qm) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
                fa[i][ks] = *(const f16x8*)(sA + swz(wr * 128 + qm * 64 + i * 16 + (lane & 15), ks * 4 + (lane >> 4)));
    };
    auto load_b = [&](const _Float16* sW, int qn) {
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
                fbq[qn][j][ks] =
                    *(const f16x8*)(sW + swz(wc * 64 + qn * 32 + j * 16 + (lane & 15), ks * 4 + (lane >> 4)));
    };
    // FIRST: the tile's first K-step starts every accumulator chain from an inline-constant 0
    // C operand, so no zeroing moves run between tiles (64 v_mov_b64 per wave and tile)
    auto compute = [&](int qm, int qn, auto firstc) {
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    f32x4& c = acc[qm * 4 + i][qn * 2 + j];
                    const f16x8& b = fbq[qn][j][ks];
                    if constexpr (decltype(firstc)::value)
                        c = mfma16(b, fa[i][ks], ks == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : c);
                    else
                        c = mfma16(b, fa[i][ks], c);
                }
    };

    // Bias of the current tile: one LDS-DMA per wave at the tile's first K-step into the
    // wave's own 1 KB slot (lane l -> bias[n0 + 4l .. 4l+3]); issued before that step's
    // B0 DMA, so the step's vmcnt(6) retires it.  The epilogue reads it with ds_read.
    const bool has_bias = EPI != EPI_PATCH && ea.bias != nullptr;
    float* bias_slot = (float*)(lds + 2 * G2_STAGE) + wid * 256;
    // Folded LayerNorm: colsum of the tile's 256 columns and (rstd, -mean rstd) of the
    // wave's 128 rows go to LDS by the same DMA at the tile's first K-step (the rowstat
    // buffer is padded to whole 256-row tiles, gemm.h).
    const bool fold = EPI != EPI_RESID_F16 && ea.rowstat != nullptr;  // (gemm_f16 rejects a residual fold)
    float* cs_slot = bias_slot + 8 * 256;
    float* rs_slot = bias_slot + 16 * 256;
    // streams: p1 = step s+1 (region B0), p2 = step s+2 (A0, B1, A1); requires nk >= 2
    Pos p1, p2;
    {
        Pos p0;
        set_tile(p0, first);
        issue_a(0, 0, p0);
        issue_a(0, 1, p0);
        issue_w(0, 0, p0);
        issue_w(0, 1, p0);
        p1 = p0;
        advance(p1);  // step 1: always inside the first tile (nk >= 2)
        issue_a(1, 0, p1);
        issue_w(1, 1, p1);
        issue_a(1, 1, p1);
        p2 = p1;
        advance(p2);
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    }
    __syncthreads();
    if (wr == 1) G5_BARRIER();
    // EPI_RRSV (rrsv_tile): record buffers and the wave's survivor buffer after the stages
    char* const rr_slot = (char*)(lds + 2 * G2_STAGE);
    const uint32_t rr_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)rr_slot;
    const uint32_t sv_lds = rr_lds + 8192 + 8192 + 8u * kRrsvWaveCap * (uint32_t)wid;
    int sv_n = 0;  // wave-uniform
    int seq = 0;   // tiles done by this workgroup
    int buf = 0;
    constexpr bool CAN_DEFER = EpiVm<EPI>::count > 0;
    bool deferred = false;  // the previous tile's epilogue stores may still be in flight
    for (int tile = first; tile < hi; tile += gx) {
        int tmt, tnt;  // this tile's M-tile and N-tile (within the group)
        tile_mn<EPI == EPI_RRSV>(tile, tnk, band, tiles_m, rr_list, tmt, tnt);
        auto kstep = [&](int kt, auto firstc) {
            const bool has1 = p1.tile < hi, has2 = p2.tile < hi;
            const bool b0_early = CAN_DEFER && kt == 0 && tile != first;  // issued before the epilogue
            const _Float16* sA = lds + buf * G2_STAGE;
            const _Float16* sW = sA + G2_M * GB_K;
            // LOAD 0 / COMPUTE (0,0)
            load_a(sA, 0);
            load_b(sW, 0);
            if (kt == 0 && has_bias)
                __builtin_amdgcn_global_load_lds(ea.bias + (nb0 + tnt) * G2_N + lane * 4, (lds_ptr_t)bias_slot,
                                                 16, 0, 0);
            if (kt == 0 && fold) {
                __builtin_amdgcn_global_load_lds(ea.colsum + (nb0 + tnt) * G2_N + lane * 4, (lds_ptr_t)cs_slot,
                                                 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const float*)(ea.rowstat + (int64_t)tmt * G2_M + wr * 128) +
                                                     lane * 4,
                                                 (lds_ptr_t)rs_slot, 16, 0, 0);
            }
            if constexpr (EPI == EPI_RRSV) {
                // this tile's row / column records (rrsv_tile), one 1 KiB piece per wave
                if (kt == 0) {
                    const int par = seq & 1;
                    if (wid < 4)
                        __builtin_amdgcn_global_load_lds(ea.rr_rowmeta + (int64_t)tmt * G2_M + wid * 64 + lane,
                                                         (lds_ptr_t)(rr_slot + par * 4096 + wid * 1024), 16, 0, 0);
                    else
                        __builtin_amdgcn_global_load_lds(ea.rr_colrec + (int64_t)(nb0 + tnt) * G2_N + (wid - 4) * 64 + lane,
                                                         (lds_ptr_t)(rr_slot + 8192 + par * 4096 + (wid - 4) * 1024),
                                                         16, 0, 0);
                }
            }
            constexpr bool KDMA = GEMM_VAR_NODMA == 0;
            if (KDMA && has1 && !b0_early) issue_w(buf ^ 1, 0, p1);
            G5_LDS_DONE();
            G5_BARRIER();
            compute(0, 0, firstc);
            G5_BARRIER();
            // LOAD 1 / COMPUTE (0,1)
            load_b(sW, 1);
            if (KDMA && has2) issue_a(buf, 0, p2);
            G5_LDS_DONE();
            G5_BARRIER();
            compute(0, 1, firstc);
            G5_BARRIER();
            // LOAD 2 / COMPUTE (1,1)
            load_a(sA, 1);
            if (KDMA && has2) issue_w(buf, 1, p2);
            G5_LDS_DONE();
            G5_BARRIER();
            compute(1, 1, firstc);
            G5_BARRIER();
            // LOAD 3 (no LDS reads: W fragments of column half 0 are still in fbq[0]) / COMPUTE (1,0)
            if (has2) {
                if constexpr (KDMA) issue_a(buf, 1, p2);
                G5_LDS_DONE();
                if constexpr (CAN_DEFER) {
                    constexpr int S = EpiVm<EPI>::count;
                    if (kt == 0 && deferred) {  // + the first K-step's bias / colsum / rowstat DMAs
                        if (fold)
                            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S + 9) : "memory");
                        else if (has_bias)
                            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S + 7) : "memory");
                        else
                            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S + 6) : "memory");
                    } else if constexpr (!GEMM_VAR_NOWAIT) {
                        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                    }
                } else if constexpr (!GEMM_VAR_NOWAIT) {
                    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                }
            } else {
                G5_LDS_DONE();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            G5_BARRIER();
            compute(1, 0, firstc);
            G5_BARRIER();
            advance(p1);
            advance(p2);
            buf ^= 1;
        };
        kstep(0, std::true_type{});  // nk >= 2 (launch: K >= 2 * GB_K)
        for (int kt = 1; kt < nk; ++kt) kstep(kt, std::false_type{});
        // both wave groups run the epilogue in the same barrier slot (group A, one barrier ahead
        // in the K-loop, waits here for group B's last COMPUTE; B catches up after it), so the
        // two groups' store tails overlap instead of running back to back
        if (wr == 0) G5_BARRIER();
        const int64_t m0 = (int64_t)tmt * G2_M;
        const int n0 = (nb0 + tnt) * G2_N;
        if constexpr (CAN_DEFER) {
            deferred = false;
            if (p1.tile < hi) {  // a next tile exists: issue its K-step 1 B0 (skipped in its LOAD 0)
                issue_w(buf ^ 1, 0, p1);
                deferred = m0 + G2_M <= M;
                if constexpr (EPI == EPI_QKV) deferred = deferred && (n0 + ea.n_off) / (ea.heads * 64) != 2;
                // the distance form's masked / unaligned stores vary in number: not deferred
                if constexpr (EPI == EPI_F32) deferred = deferred && ea.dist_rsq == nullptr;
            }
        }
        // residual epilogue: its row reads go out before the bias arithmetic (after the next
        // tile's early DMA, so the deferred-store count EpiVm is unchanged), their latency
        // then runs beside it
        constexpr bool RPRE = EPI == EPI_RESID_F16 && !GEMM_VAR_NORESLOAD;
        f16x8 xres[RPRE ? 8 : 1][2];
        if constexpr (RPRE) resid_rows_load<8>(ea, m0 + wr * 128, n0 + wc * 64, M, xres);
        if (has_bias) {
            f32x4 b[4];
            // inline ds_read: no compiler-inserted vmcnt(0) for the LDS-DMA'd slot (retired by
            // the tile's first K-step wait)
            const float* bp = bias_slot + wc * 64 + (lane >> 4) * 4;
            const uint32_t ba = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)bp;
            asm volatile("ds_read_b128 %0, %1" : "=v"(b[0]) : "v"(ba) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(b[1]) : "v"(ba) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(b[2]) : "v"(ba) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:192" : "=v"(b[3]) : "v"(ba) : "memory");
            // the wait names the read registers: no use of them can be scheduled above it (the
            // hardware does not track VGPRs written by an outstanding LDS read)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])::"memory");
            // acc <- rstd * acc + (-mean rstd * s_n + b'_n); without a fold (rstd, s) = (1, 0):
            // fma(1, acc, fma(0, 0, b)) == acc + b exactly.  One branch-free update (a branch on
            // acc would duplicate the 128 accumulators).
            f32x4 sn[4];
            f32x2v rs[8];
            if (fold) {
                const uint32_t ca = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)(
                    cs_slot + wc * 64 + (lane >> 4) * 4);
                const uint32_t ra =
                    (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)(rs_slot + (lane & 15) * 2);
                asm volatile("ds_read_b128 %0, %1" : "=v"(sn[0]) : "v"(ca) : "memory");
                asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(sn[1]) : "v"(ca) : "memory");
                asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(sn[2]) : "v"(ca) : "memory");
                asm volatile("ds_read_b128 %0, %1 offset:192" : "=v"(sn[3]) : "v"(ca) : "memory");
                asm volatile("ds_read_b64 %0, %1" : "=v"(rs[0]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:128" : "=v"(rs[1]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:256" : "=v"(rs[2]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:384" : "=v"(rs[3]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:512" : "=v"(rs[4]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:640" : "=v"(rs[5]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:768" : "=v"(rs[6]) : "v"(ra) : "memory");
                asm volatile("ds_read_b64 %0, %1 offset:896" : "=v"(rs[7]) : "v"(ra) : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(sn[0]), "+v"(sn[1]), "+v"(sn[2]), "+v"(sn[3]), "+v"(rs[0]), "+v"(rs[1]), "+v"(rs[2]),
                               "+v"(rs[3]), "+v"(rs[4]), "+v"(rs[5]), "+v"(rs[6]), "+v"(rs[7])::"memory");
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) sn[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 8; i++) rs[i] = f32x2v{1.f, 0.f};
            }
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    acc[i][j][0] = __builtin_fmaf(rs[i].x, acc[i][j][0], __builtin_fmaf(rs[i].y, sn[j].x, b[j].x));
                    acc[i][j][1] = __builtin_fmaf(rs[i].x, acc[i][j][1], __builtin_fmaf(rs[i].y, sn[j].y, b[j].y));
                    acc[i][j][2] = __builtin_fmaf(rs[i].x, acc[i][j][2], __builtin_fmaf(rs[i].y, sn[j].z, b[j].z));
                    acc[i][j][3] = __builtin_fmaf(rs[i].x, acc[i][j][3], __builtin_fmaf(rs[i].y, sn[j].w, b[j].w));
                }
        }
        if constexpr (EPI == EPI_RRSV)
            rrsv_tile(ea, acc, m0 + wr * 128, n0 + wc * 64, M, seq, ea.rr_tri && tmt < tnt, rr_lds + (seq & 1) * 4096,
                      rr_lds + 8192 + (seq & 1) * 4096, sv_lds, sv_n, lane,
                      RrsvWalk{first, gx, wr, wc, rr_list});
        else if (EPI == EPI_GELU_H16 && m0 + G2_M <= M)  // c_fc's full tiles: no row checks
            epilogue_tile<EPI, 8, true, RPRE, true>(ea, acc, m0 + wr * 128, n0 + wc * 64, M, N, xres);
        else
            epilogue_tile<EPI, 8, true, RPRE>(ea, acc, m0 + wr * 128, n0 + wc * 64, M, N, xres);
        seq++;
        if (wr == 1) G5_BARRIER();
    }
    if constexpr (EPI == EPI_RRSV)
        rrsv_flush(ea, sv_lds, sv_n, lane, RrsvWalk{first, gx, wr, wc, rr_list});
    if (wr == 0) G5_BARRIER();
#undef G5_BARRIER
#undef G5_LDS_DONE
}

template <int EPI>
static int launch(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K,
                  const EpiArgs& ea, hipStream_t s, const GemmOpts& opt) {
    const bool listed = EPI == EPI_RRSV;  // walks a tile list (gemm.h rr_tiles)
    RM_REQUIRE(!listed || (ea.rr_tiles && ea.rr_ntiles > 0), "gemm: the survivor epilogue needs its tile list");
    const int64_t tiles256 = listed ? ea.rr_ntiles : (int64_t)ceil_div(M, G2_M) * (N / G2_N);
    const bool fits = N % G2_N == 0 && K >= 2 * GB_K && lda * G2_M < (1ll << 31) && ldw * G2_N < (1ll << 31);
    if (fits && (opt.tile == 2 || (opt.tile == 0 && tiles256 >= 256))) {
        // a tile list is walked as tiles_m = its length x 1 N-tile, one XCD group
        const int tiles_m = listed ? (int)tiles256 : ceil_div(M, G2_M), tiles_n = listed ? 1 : (int)(N / G2_N);
        RM_REQUIRE(tiles256 < (1ll << 31), "gemm: grid too large");
        RM_REQUIRE(!listed || (ceil_div(M, G2_M) <= 65536 && N / G2_N <= 65536), "gemm: tile list: too many tiles");
        RM_REQUIRE(EPI != EPI_RRSV || tiles256 / (tiles256 < 256 ? tiles256 : 256) < (1 << 18),
                   "gemm: survivor epilogue: too many tiles per workgroup");
        // two operand stages + bias / colsum / rowstat slots (8 waves x 1 KiB each)
        // (EPI_RRSV: its record and survivor buffers instead, rrsv_tile)
        const size_t lds = 2 * (size_t)G2_STAGE * 2 + (EPI == EPI_RRSV ? kRrsvSlotBytes : 3 * 8 * 256 * sizeof(float));
        // c_proj (residual epilogue, K > N) launches the TAG 1 copy of the kernel
        const bool tag1 = EPI == EPI_RESID_F16 && K > N;
        auto kern = tag1 ? gemm_persistent_kernel<EPI, EPI == EPI_RESID_F16 ? 1 : 0> : gemm_persistent_kernel<EPI, 0>;
        static bool attr[2] = {false, false};
        if (!attr[tag1]) {
            RM_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr[tag1] = true;
        }
        const int grid = (int)(tiles256 < 256 ? tiles256 : 256);
        // XCD N-groups: auto = 2 when the N-tiles split evenly and there are >= 8 of them
        // (c_fc: 12 tiles, +2 %, 15 % less L2 fetch; an uneven split idles the XCDs of the
        // smaller group), else 1 (profiles/r02/walk_ab.txt)
        const int ngroups =
            listed ? 1 : opt.ngroups > 0 ? opt.ngroups : (tiles_n % 2 == 0 && tiles_n >= 8 ? 2 : 1);
        // bands of M-tiles: auto = 8 for the re-rank's dense N x N product (both operands
        // stream from HBM; the survivor epilogue's tile list is in band order too), else
        // M-major (the encoder's weights stay in L2 / MALL)
        const int band = EPI != EPI_RRHI ? 0 : opt.band >= 0 ? opt.band : RR_GEMM_BAND;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), lds, s, (const _Float16*)A,
                           lda, (const _Float16*)W, ldw, M, (int)N, (int)K, ea, tiles_m, tiles_n, ngroups, band);
        RM_LAUNCHED();
        return OK;
    }
    if constexpr (EPI == EPI_RRSV) {
        return fail(EINVAL_, "gemm: the survivor epilogue runs on the persistent 256 x 256 tile only "
                             "(N % 256 == 0, K >= 128, >= 256 tiles)");
    } else {
    const int tiles_m = ceil_div(M, GB_M), tiles_n = (int)(N / GB_N);
    const int64_t nwg = (int64_t)tiles_m * tiles_n;
    RM_REQUIRE(nwg < (1ll << 31), "gemm: grid too large");
    hipLaunchKernelGGL((gemm_tile_kernel<EPI>), dim3((unsigned)nwg), dim3(256), 0, s, (const _Float16*)A, lda,
                       (const _Float16*)W, ldw, M, (int)N, (int)K, ea, tiles_n, (int)nwg);
    RM_LAUNCHED();
    return OK;
    }
}

int gemm_f16(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K,
             const EpiArgs& ea, hipStream_t s, const GemmOpts& opt) {
    RM_REQUIRE(opt.tile >= 0 && opt.tile <= 2, "gemm tile: 0 auto, 1 128x128, 2 persistent 256x256");
    RM_REQUIRE(opt.band >= -1 && opt.band <= 64, "gemm walk: band in -1 (auto) .. 64");
    RM_REQUIRE(opt.ngroups == 0 || opt.ngroups == 1 || opt.ngroups == 2 || opt.ngroups == 4 || opt.ngroups == 8,
               "gemm walk: ngroups in {0 (auto), 1, 2, 4, 8}");
    RM_REQUIRE(M >= 0 && N > 0 && K > 0, "gemm: bad shape");
    RM_REQUIRE((epi != EPI_QKV && epi != EPI_PATCH) || M < (1ll << 31), "gemm: head split / patch rows need M < 2^31");
    RM_REQUIRE(N % GB_N == 0 && K % GB_K == 0, "gemm: needs N % 128 == 0 and K % 64 == 0");
    RM_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K, "gemm: lda/ldw must be >= K and 16-byte rows");
    RM_REQUIRE((epi != EPI_H16 && epi != EPI_GELU_H16 && epi != EPI_RESID_F16) ||
                   (ea.ldc % 8 == 0 && ((uintptr_t)ea.out & 15) == 0 && ea.ldc < (1 << 24) && N < (1 << 24)),
               "gemm: fp16 output needs ldc % 8 == 0 (< 2^24) and a 16-byte aligned base");
    RM_REQUIRE((ea.rowstat == nullptr) == (ea.colsum == nullptr), "gemm: rowstat and colsum go together");
    RM_REQUIRE(ea.rowstat == nullptr || ea.bias != nullptr, "gemm: a folded LayerNorm needs the folded bias");
    RM_REQUIRE(epi != EPI_RESID_F16 || ea.rowstat == nullptr, "gemm: the residual epilogue takes no folded LayerNorm");
    RM_REQUIRE(ea.dist_rsq == nullptr || (epi == EPI_F32 && ea.dist_csq != nullptr && ea.dist_n > 0 &&
                                          ea.dist_n <= N && ea.ldc >= ea.dist_n && ea.bias == nullptr),
               "gemm: the distance form needs EPI_F32, both norm vectors, 0 < dist_n <= N, ldc >= dist_n, no bias");
    if (M == 0) return OK;
    hipEvent_t ev_b = nullptr;
    if (prof::enabled) {
        std::lock_guard<std::mutex> g(prof::mu);
        if (prof::used == prof::pool.size()) {
            hipEvent_t a, b;
            RM_CHECK_HIP(hipEventCreate(&a));
            RM_CHECK_HIP(hipEventCreate(&b));
            prof::pool.push_back({a, b});
        }
        auto pr = prof::pool[prof::used++];
        prof::recs.push_back({pr.first, pr.second, 2.0 * (double)M * (double)N * (double)K, epi});
        RM_CHECK_HIP(hipEventRecord(pr.first, s));
        ev_b = pr.second;
    }
    int rc;
    switch (epi) {
        case EPI_H16: rc = launch<EPI_H16>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_GELU_H16: rc = launch<EPI_GELU_H16>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_QKV: rc = launch<EPI_QKV>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_PATCH: rc = launch<EPI_PATCH>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_F32: rc = launch<EPI_F32>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_RESID_F16: rc = launch<EPI_RESID_F16>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_RRHI: rc = launch<EPI_RRHI>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        case EPI_RRSV: rc = launch<EPI_RRSV>(A, lda, W, ldw, M, N, K, ea, s, opt); break;
        default: return fail(EINVAL_, "gemm: unknown epilogue");
    }
    if (ev_b) RM_CHECK_HIP(hipEventRecord(ev_b, s));
    return rc;
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_prof_enable(int on) {
    std::lock_guard<std::mutex> g(prof::mu);
    prof::enabled = on != 0;
    prof::recs.clear();
    prof::used = 0;
    return OK;
}

// Sum of device time (ms), launch count and algorithmic FLOPs of the recorded GEMM launches
// with epilogue `epi` (-1: all) and at least `min_flops` each.  Waits for the recorded
// events; then clears the record.
REIDMI_API int reidmi_prof_collect_min(int epi, double min_flops, double* total_ms, int64_t* count, double* flops) {
    std::lock_guard<std::mutex> g(prof::mu);
    double t = 0, f = 0;
    int64_t n = 0;
    for (auto& r : prof::recs) {
        if (epi >= 0 && r.epi != epi) continue;
        if (r.flops < min_flops) continue;
        RM_CHECK_HIP(hipEventSynchronize(r.b));
        float ms = 0;
        RM_CHECK_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        t += ms;
        f += r.flops;
        n++;
    }
    if (total_ms) *total_ms = t;
    if (count) *count = n;
    if (flops) *flops = f;
    prof::recs.clear();
    prof::used = 0;
    return OK;
}

REIDMI_API int reidmi_prof_collect(int epi, double* total_ms, int64_t* count, double* flops) {
    return reidmi_prof_collect_min(epi, 0.0, total_ms, count, flops);
}

static int gemm_api(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K,
                    const float* bias, const void* rowstat, const float* colsum, void* out, int64_t ldc,
                    const GemmOpts& opt, void* stream) {
    RM_REQUIRE(epi == EPI_H16 || epi == EPI_GELU_H16 || epi == EPI_F32 || epi == EPI_RESID_F16,
               "reidmi_gemm_f16: epi must be 0 (fp16), 1 (QuickGELU fp16), 5 (fp32) or 6 (fp16 residual)");
    EpiArgs ea{};
    ea.out = out;
    ea.ldc = ldc;
    ea.bias = bias;
    ea.rowstat = (const float2*)rowstat;
    ea.colsum = colsum;
    return gemm_f16(epi, A, lda, W, ldw, M, N, K, ea, (hipStream_t)stream, opt);
}

REIDMI_API int reidmi_gemm_f16(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N,
                               int64_t K, const float* bias, const void* rowstat, const float* colsum, void* out,
                               int64_t ldc, void* stream) {
    return gemm_api(epi, A, lda, W, ldw, M, N, K, bias, rowstat, colsum, out, ldc, GemmOpts{}, stream);
}

#ifdef REIDMI_TOOLS
// ================================================ one-wave-per-SIMD prototype (W4, tools only)
// The next GEMM design of DESIGN.md §5 (design (c), hipBLASLt's shape), measured before it is
// built out: 256 threads = 4 waves, one per SIMD (up to 512 registers each), 256 x 256 x 64
// tile; wave (wr, wc) owns rows 128 wr.. and columns 128 wc.. (8 x 8 fragments of 16 x 16:
// 256 accumulator registers).  Two LDS stages; the next K-step's operands are DMA'd during the
// current one (16 one-KiB pieces per wave, one per 8 MFMAs); one barrier per K-step.  Same
// MFMA chain per output element as gemm_persistent_kernel (bit-identical).  Plain fp16 +
// bias epilogue (NOSTORE: values kept, no stores) — a mainloop measurement.
#ifndef W4_VAR_NODMA  // timing variants of the prototype (wrong results): no operand DMA in the K-loop
#define W4_VAR_NODMA 0
#endif
#ifndef W4_VAR_NOWAIT  // ... the DMA issued but never waited for in the K-loop
#define W4_VAR_NOWAIT 0
#endif
#ifndef W4_VAR_NOBARRIER  // ... no barrier per K-step
#define W4_VAR_NOBARRIER 0
#endif
namespace reidmi {
template <bool NOSTORE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm_w4_kernel(
    const _Float16* __restrict__ A, int64_t lda, const _Float16* __restrict__ W, int64_t ldw, int64_t M, int N, int K,
    EpiArgs ea, int tiles_n, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
    constexpr int STAGE = (G2_M + G2_N) * GB_K;  // fp16 elements: A 256 x 64, then W 256 x 64
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    const int nk = K / GB_K;
    const int G = gridDim.x;
    // DMA: waves 0, 1 bring A (pieces of 8 rows x 128 B), waves 2, 3 bring W; 16 pieces each.
    // Piece u covers rows prow0 + 8u + (lane >> 3); its source chunk is swizzled by
    // ((row >> 1) & 7) = (4u + (lane >> 4)) & 7: two per-lane chunk offsets (u even / odd).
    // Every K-step issues all 16 pieces (past the workgroup's last K-step they re-read a valid
    // K-step into the stage nobody reads again): no branches in the loop.
    const bool isA = wid < 2;
    const int prow0 = (wid & 1) * 128;
    const int ld = (int)(isA ? lda : ldw);
    const int l3 = lane >> 3;
    const uint32_t chk_e = (uint32_t)(((lane & 7) ^ ((l3 >> 1) & 7)) << 3);
    const uint32_t chk_o = (uint32_t)(((lane & 7) ^ (((l3 >> 1) + 4) & 7)) << 3);
    _Float16* const dst0 = lds + (isA ? 0 : G2_M * GB_K) + prow0 * GB_K;
    f32x4 accL[8][4], accR[8][4];  // columns wc*128 + [0, 64) and [64, 128)
    f16x8 fa[8], fb[2][8];         // A fragments of one k-half (reused per row group), W of both
    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    // source of K-step kt of tile t for this wave's 128 operand rows, and how many of them exist
    auto src_of = [&](int t, int kt, int& lim) -> const _Float16* {
        const int64_t m0 = (int64_t)(t / tiles_n) * G2_M;
        const int n0 = (t % tiles_n) * G2_N;
        if (isA) {
            const int64_t left = M - m0 - prow0;
            lim = left < 128 ? (int)(left > 0 ? left : 1) : 128;
            return A + (m0 + (left > 0 ? prow0 : 0)) * lda + kt * GB_K;
        }
        lim = 128;
        return W + ((int64_t)n0 + prow0) * ldw + kt * GB_K;
    };
    // SGPR base + unsigned VGPR byte offset per piece (no 64-bit VALU address arithmetic): a
    // piece past the matrix's last row reads the last 8 rows (or, with fewer than 8, the last
    // row in every lane) -- valid addresses; those rows are never stored
    const uint32_t loff_e = (uint32_t)(l3 * ld + (int)chk_e) * 2u, loff_o = (uint32_t)(l3 * ld + (int)chk_o) * 2u;
    auto issue = [&](const _Float16* src, int lim, int stage, int u) {
        const bool whole = 8 * u + 8 <= lim;  // wave-uniform
        const int brow = whole ? 8 * u : (lim >= 8 ? lim - 8 : lim - 1);
        const uint32_t voff = (whole || lim >= 8) ? ((u & 1) ? loff_o : loff_e) : ((u & 1) ? chk_o : chk_e) * 2u;
        __builtin_amdgcn_global_load_lds((const char*)(src + (int64_t)brow * ld) + voff,
                                         (lds_ptr_t)(dst0 + stage * STAGE + 8 * u * GB_K), 16, 0, 0);
    };
    auto read_b = [&](const _Float16* sW, int ks, int b) {
#pragma unroll
        for (int j = 0; j < 8; j++)
            fb[b][j] = *(const f16x8*)(sW + swz(wc * 128 + j * 16 + (lane & 15), ks * 4 + (lane >> 4)));
    };
    auto read_a = [&](const _Float16* sA, int ks, int i) {
        fa[i] = *(const f16x8*)(sA + swz(wr * 128 + i * 16 + (lane & 15), ks * 4 + (lane >> 4)));
    };
    // prologue: K-step 0 of the first tile
    {
        int lim;
        const _Float16* src = src_of(tile, 0, lim);
#pragma unroll
        for (int u = 0; u < 16; u++) issue(src, lim, 0, u);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int buf = 0;
    for (; tile < ntiles; tile += G) {
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) accL[i][j] = accR[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < nk; kt++) {
            // the next K-step in the workgroup's stream (this tile's, or the next tile's first)
            const bool last = kt + 1 == nk;
            const int nt = last && tile + G < ntiles ? tile + G : tile;
            const int nkt = last ? 0 : kt + 1;
            int nlim;
            const _Float16* nsrc = src_of(nt, nkt, nlim);
            const _Float16* sA = lds + buf * STAGE;
            const _Float16* sW = sA + G2_M * GB_K;
            read_b(sW, 0, 0);
#pragma unroll
            for (int i = 0; i < 8; i++) read_a(sA, 0, i);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            // k-half 0: row group g's MFMAs, then its A fragment of k-half 1 (the register is
            // free after them); W of k-half 1 read behind group 0; one DMA piece per group
#pragma unroll
            for (int g = 0; g < 8; g++) {
                if (!W4_VAR_NODMA) issue(nsrc, nlim, buf ^ 1, g);
                if (g == 0) read_b(sW, 1, 1);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    accL[g][j] = mfma16(fb[0][j], fa[g], accL[g][j]);
                    accR[g][j] = mfma16(fb[0][4 + j], fa[g], accR[g][j]);
                }
                read_a(sA, 1, g);
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int g = 0; g < 8; g++) {
                if (!W4_VAR_NODMA) issue(nsrc, nlim, buf ^ 1, 8 + g);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    accL[g][j] = mfma16(fb[1][j], fa[g], accL[g][j]);
                    accR[g][j] = mfma16(fb[1][4 + j], fa[g], accR[g][j]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // the next K-step's operands landed (every wave's: barrier); this stage is free
            if (!W4_VAR_NOWAIT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (!W4_VAR_NOBARRIER) __builtin_amdgcn_s_barrier();
            buf ^= 1;
        }
        const int64_t m0 = (int64_t)(tile / tiles_n) * G2_M;
        const int n0 = (tile % tiles_n) * G2_N;
        if constexpr (NOSTORE) {
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) asm volatile("" ::"v"(accL[i][j]), "v"(accR[i][j]));
        } else {
            epilogue_tile<EPI_H16, 8>(ea, accL, m0 + wr * 128, n0 + wc * 128, M, N);
            epilogue_tile<EPI_H16, 8>(ea, accR, m0 + wr * 128, n0 + wc * 128 + 64, M, N);
        }
    }
}
}  // namespace reidmi

REIDMI_API int reidmi_gemm_f16_w4(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N,
                                  int64_t K, const float* bias, void* out, int64_t ldc, int nostore, void* stream) {
    RM_REQUIRE(M > 0 && N % G2_N == 0 && K % GB_K == 0 && K >= 2 * GB_K, "gemm_w4: needs N % 256 == 0, K % 64 == 0");
    RM_REQUIRE(nostore == 0 || nostore == 1, "gemm_w4: nostore is 0 or 1");
    RM_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && ldc % 8 == 0 && lda * G2_M < (1ll << 31) && ldw * G2_N < (1ll << 31),
               "gemm_w4: strides");
    const int tiles_n = (int)(N / G2_N);
    const int64_t ntiles = (int64_t)ceil_div(M, G2_M) * tiles_n;
    RM_REQUIRE(ntiles < (1ll << 31), "gemm_w4: too many tiles");
    EpiArgs ea{};
    ea.out = out;
    ea.ldc = ldc;
    ea.bias = bias;
    const size_t lds = 2 * (size_t)(G2_M + G2_N) * GB_K * 2;
    auto kern = nostore ? gemm_w4_kernel<true> : gemm_w4_kernel<false>;
    RM_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int grid = (int)(ntiles < 256 ? ntiles : 256);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, (const _Float16*)A, lda,
                       (const _Float16*)W, ldw, M, (int)N, (int)K, ea, tiles_n, (int)ntiles);
    RM_LAUNCHED();
    return OK;
}

// Forced tiling / walk (tests, A-B timing; tools library, include/reidmi_tools.h)
REIDMI_API int reidmi_gemm_f16_tiled(int epi, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M,
                                     int64_t N, int64_t K, const float* bias, const void* rowstat, const float* colsum,
                                     void* out, int64_t ldc, int tile, int ngroups, void* stream) {
    GemmOpts opt;
    opt.tile = tile;
    opt.ngroups = ngroups;
    return gemm_api(epi, A, lda, W, ldw, M, N, K, bias, rowstat, colsum, out, ldc, opt, stream);
}

// The QKV GEMM alone (EPI_QKV: ln_1 fold + head split into q, k [nseq*H][L][64] and
// v^T [nseq*H][64][lpad]): columns [n_off, n_off + N) of [q | k | v] (W, bias and colsum point at
// the first of them, as run_block_cls passes them), with the tiling of opt
static int qkv_api(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t nseq, int L, int H, int64_t N,
                   int64_t n_off, const float* bias, const void* rowstat, const float* colsum, void* q, void* k,
                   void* vt, int lpad, const GemmOpts& opt, void* stream) {
    const int64_t wd = (int64_t)H * 64;
    RM_REQUIRE(nseq >= 0 && L > 0 && H > 0 && lpad >= L, "gemm_f16_qkv: bad shape");
    RM_REQUIRE(N > 0 && n_off >= 0 && n_off % 64 == 0 && n_off + N <= 3 * wd, "gemm_f16_qkv: columns outside [q | k | v]");
    RM_REQUIRE((q || n_off >= wd) && (k || n_off >= 2 * wd || n_off + N <= wd) && (vt || n_off + N <= 2 * wd),
               "gemm_f16_qkv: null output for a produced column block");
    EpiArgs ea{};
    ea.bias = bias;
    ea.rowstat = (const float2*)rowstat;
    ea.colsum = colsum;
    ea.q = q;
    ea.k = k;
    ea.vt = vt;
    ea.seq = L;
    ea.heads = H;
    ea.lpad = lpad;
    ea.n_off = (int)n_off;
    return gemm_f16(EPI_QKV, A, lda, W, ldw, nseq * L, N, wd, ea, (hipStream_t)stream, opt);
}

// ... the whole [q | k | v], automatic tiling, for pricing its epilogue against a plain fp16
// output (tools/lib_ab.py)
REIDMI_API int reidmi_gemm_f16_qkv(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t nseq, int L, int H,
                                   const float* bias, const void* rowstat, const float* colsum, void* q, void* k,
                                   void* vt, int lpad, void* stream) {
    return qkv_api(A, lda, W, ldw, nseq, L, H, 3 * (int64_t)H * 64, 0, bias, rowstat, colsum, q, k, vt, lpad,
                   GemmOpts{}, stream);
}

// ... any column range and a forced tiling (tests: the K / V-only and CLS-query forms of run_block_cls)
REIDMI_API int reidmi_gemm_f16_qkv_ex(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t nseq, int L,
                                      int H, int64_t N, int64_t n_off, const float* bias, const void* rowstat,
                                      const float* colsum, void* q, void* k, void* vt, int lpad, int tile, int ngroups,
                                      void* stream) {
    GemmOpts opt;
    opt.tile = tile;
    opt.ngroups = ngroups;
    return qkv_api(A, lda, W, ldw, nseq, L, H, N, n_off, bias, rowstat, colsum, q, k, vt, lpad, opt, stream);
}
#endif  // REIDMI_TOOLS
