// attention.h — the attention host interface (for encoder.hip and resnet.hip) and the device
// pieces the attention kernels share (attention.hip: the whole-head kernels for L <= 256;
// attention_long.hip: the streamed-key kernels for L <= 1024): the Q prefetch, the K swizzle in
// LDS, the accumulator key index, the fp16 conversions, the cross-half exchanges, the O store.
#pragma once
#include "common.h"

namespace reidmi {

// host interface: longest sequence of attention.hip's whole-head kernels (mhsa, mhsa_cls); longer ones, up to
// kAttnLongMax, take attention_long.hip's streamed-key kernels (vision only, non-causal).
constexpr int kAttnShortMax = 256, kAttnLongMax = 1024;
// exp(x / sqrt(64)) = exp2(x * kAttnScaleLog2): 1/sqrt(64) * log2(e)
constexpr float kAttnScaleLog2 = 0.125f * 1.4426950408889634f;

// V^T row stride (elements) of an L-token sequence: LP + 4 with LP = L rounded up to 32-key
// blocks, i.e. LP/2 + 2 dwords, which is 2 mod 4 dwords: the 32 rows of one half-wave
// ds_read_b64 then start on 32 distinct even banks (row r at bank 2 * (r * odd mod 32)), so they
// cover all 64 banks exactly once.  (The stride 2 mod 64 used before padded V^T by up to 60
// elements per row: 23 % of V at L = 211.)  The QKV epilogue writes V^T with this same stride in
// HBM, so one head's V^T is a contiguous blob for the LDS-DMA copy; 64 * (LP + 4) * 2 bytes is a
// multiple of 512.
constexpr int vt_stride(int L) { return (L + 31) / 32 * 32 + 4; }
inline int attn_vt_stride(int L) { return L < 1 || L > kAttnLongMax ? -1 : vt_stride(L); }
inline int attn_lpad(int L) { return L <= kAttnShortMax ? attn_vt_stride(L) : -1; }  // the whole-head kernels' range

// q, k [nseq*H][L][64], vt [nseq*H][64][attn_vt_stride(L)] -> o [nseq*L][H*64], all fp16; the _cls
// forms take the CLS query only, q [nseq*H][64] -> o [nseq][H*64]; attn / attn_cls pick by length
int mhsa(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H, bool causal, hipStream_t s);
int mhsa_long(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H, hipStream_t s);
int attn(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H, bool causal, hipStream_t s);
int mhsa_cls(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H, hipStream_t s);
int mhsa_cls_long(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H, hipStream_t s);
int attn_cls(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H, hipStream_t s);
int64_t cls_attn_nokv_ws_bytes(int64_t nseq, int W);
int cls_attn_nokv(const void* x, const void* rs, const void* q, const void* wqkv, const float* colsum,
                  const float* bias, int64_t nseq, int L, int H, int W, void* ws, void* o, hipStream_t s);

// ------------------------------------------------------------------------- device pieces
typedef __attribute__((address_space(3))) void* lds_ptr_t;
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

// The 64 halves at qh + 0, 16, 32, 48 (a lane's four B fragments of its Q row) as inline-asm
// loads: hipcc does not track them, so it inserts no vmcnt(0) of its own before the registers
// are used (which would also drain the O stores and the LDS-DMA in flight).  The kernel's own
// counted s_waitcnt retires them, and pin_q4 after that wait orders every use behind it.
__device__ __forceinline__ void load_q4(const _Float16* qh, f16x8 (&qf)[4]) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qf[0]) : "v"(qh) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, off offset:32" : "=v"(qf[1]) : "v"(qh) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, off offset:64" : "=v"(qf[2]) : "v"(qh) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, off offset:96" : "=v"(qf[3]) : "v"(qh) : "memory");
}
__device__ __forceinline__ void pin_q4(f16x8 (&qf)[4]) {
    asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]));
}

// K [rows][64] fp16 in LDS: the 16-byte chunk kc of row r sits at chunk kc ^ ((r >> 1) & 7)
__device__ __forceinline__ int kswz_chunk(int r, int kc) { return kc ^ ((r >> 1) & 7); }
__device__ __forceinline__ int kswz(int r, int kc) { return r * 64 + (kswz_chunk(r, kc) << 3); }

// Accumulator register r of lane (ql = lane & 31, hh = lane >> 5) after S^T = K Q^T of a 32-key
// block (v_mfma_f32_32x32x16_f16) is key acc_key(r, hh) of the block, for query ql
__device__ __forceinline__ int acc_key(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));

// fp32 -> fp16 (RNE) of a value that must be rounded to fp32 first: the opaque copy keeps the
// backend from merging the fma that produced x and this conversion into one v_fma_mixlo_f16
// (a single rounding to fp16, which differs from gemm.hip's in about 1 value in 1500)
__device__ __forceinline__ _Float16 f32_to_h(float x) {
    asm("" : "+v"(x));
    return (_Float16)x;
}

// one v_cvt_pk_f16_f32 (RNE) per pair, as gemm.hip's epilogues convert
__device__ __forceinline__ uint32_t cvt_pk_h(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2v{a, b}, f16x2v));
}

// fp16 pair (a * inv, b * inv), each product rounded to fp16 ONCE (v_fma_mixlo / mixhi: the
// exact product, one rounding).  Left to itself the backend lowers (_Float16)(a * inv) as a
// mix instruction for some elements and as v_mul + v_cvt_pk (two roundings) for others, so
// the two attention blocks would differ in ~1 value in 36 000.
__device__ __forceinline__ uint32_t mul_pk_h(float a, float b, float inv) {
#ifdef ATTN_OUT_CVT  // A/B only: fp32 product, then RNE to fp16 (two roundings)
    float x = a * inv, y = b * inv;
    asm("" : "+v"(x), "+v"(y));
    return cvt_pk_h(x, y);
#endif
    uint32_t r;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(inv));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(r) : "v"(b), "v"(inv));
    return r;
}

// {x[l], x[l ^ 32]} in some order per lane.  The results are copied out as uint32_t before any
// bit_cast: hipcc 7.2 lowers __builtin_bit_cast(float, r[1]) applied to the builtin's vector
// result as element 0 (both results then read the first register).
__device__ __forceinline__ void xhalf_pair(float x, float& a, float& b) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const uint32_t r0 = r[0], r1 = r[1];
    a = __builtin_bit_cast(float, r0);
    b = __builtin_bit_cast(float, r1);
}
__device__ __forceinline__ float xhalf_max(float x) {  // max(x[l], x[l ^ 32])
    float a, b;
    xhalf_pair(x, a, b);
    return fmaxf(a, b);
}
__device__ __forceinline__ float xhalf_sum(float x) {  // x[l] + x[l ^ 32] (commutative: = x + shfl_xor(x, 32))
    float a, b;
    xhalf_pair(x, a, b);
    return a + b;
}

// O^T[d][q] * inv of one 32-query block -> o [nseq*L][H*64] fp16, each element rounded once
// (mul_pk_h).  Lane (ql, hh) holds d = db*32 + 8g + 4hh + 0..3 of query qi in oacc[db][4g..4g+3];
// pairs g = 2j, 2j+1 are exchanged across the halves (one v_permlane32_swap per dword) so that
// half 0 stores d 16j..16j+7 and half 1 d 16j+8..16j+15: kAttnPipeStores 16-byte stores per lane.
// Lanes with qi >= L store nothing.
constexpr int kAttnPipeStores = 4;
__device__ __forceinline__ void store_o_wide(const f32x16 (&oacc)[2], float inv, int qi, int hh, int L, int64_t bh,
                                             int H, _Float16* __restrict__ o) {
    uint4 w[2][2];
#pragma unroll
    for (int db = 0; db < 2; db++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int g0 = 2 * j, g1 = 2 * j + 1;
            auto pk = [&](int e) { return mul_pk_h(oacc[db][e], oacc[db][e + 1], inv); };
            const uint32_t x0 = pk(4 * g0), x1 = pk(4 * g0 + 2), y0 = pk(4 * g1), y1 = pk(4 * g1 + 2);
            const auto r0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
            const auto r1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
            w[db][j] = make_uint4(r0[0], r1[0], r0[1], r1[1]);
        }
    if (qi < L) {
        const int64_t b = bh / H, hd = bh % H;
        _Float16* orow = o + (b * L + qi) * (int64_t)(H * 64) + hd * 64 + 8 * hh;
        static_assert(2 * 2 == kAttnPipeStores, "one store per (d block, pair)");
#pragma unroll
        for (int db = 0; db < 2; db++)
#pragma unroll
            for (int j = 0; j < 2; j++) *(uint4*)(orow + db * 32 + 16 * j) = w[db][j];
    }
}

}  // namespace reidmi
