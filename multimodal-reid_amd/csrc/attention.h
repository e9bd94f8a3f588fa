// attention.h — the pieces the attention kernels share (attention.hip: the whole-head kernels
// for L <= 256; attention_long.hip: the streamed-key kernels for L <= 1024): the K swizzle in
// LDS, the single-rounding fp16 conversions, the cross-half exchanges and the widened O store.
#pragma once
#include "common.h"

namespace reidmi {

// K [rows][64] fp16 in LDS: the 16-byte chunk kc of row r sits at chunk kc ^ ((r >> 1) & 7)
__device__ __forceinline__ int kswz(int r, int kc) { return r * 64 + ((kc ^ ((r >> 1) & 7)) << 3); }

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
