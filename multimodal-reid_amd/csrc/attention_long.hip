// attention_long.hip — streamed-key attention for the vision tower beyond 256 tokens (gfx950).
//
// Non-causal softmax(Q K^T / sqrt(64)) V per (sequence, head) for 1 <= L <= 1024: square and
// large input crops (224 x 224 -> 325 tokens, 256 x 256 -> 442, 384 x 384 -> 962 on the
// stride-12 ViT-B/16 grid).  attention.hip keeps the whole K and V^T of a head in LDS and all
// of a row's scores in registers, which ends at 256 keys; here K and V^T pass through LDS in
// tiles of kLongTile keys and each query row keeps a running max and sum (online softmax).
// Same layouts as attention.hip (q, k [nseq*H][L][64], vt [nseq*H][64][stride], o
// [nseq*L][H*64], fp16) and the same rounding points: fp32 scores, exponentials, sums and
// accumulation, P rounded to fp16 once for the P.V MFMAs, O rounded to fp16 once (mul_pk_h).
#include "attention.h"

namespace reidmi {

// One workgroup = kLongWaves waves = kLongWaves consecutive 32-query blocks of one head; the
// workgroups of a head (ceil(L / 128)) are neighbours in the grid, so the head's K and V^T come
// from L2 for all but the first.  Per key tile (kLongTile = 64 keys = two 32-key blocks):
//   * all 256 threads copy the next tile's K rows (16-byte pieces, XOR-swizzled as in
//     attention.hip) and V^T columns (8-byte pieces: a V^T row starts on an 8-byte boundary only)
//     into registers before the tile's MFMAs and into the other LDS stage after them: one
//     barrier per tile.  K rows >= L repeat row L-1 (finite; their scores are masked to -inf).
//     V^T columns >= L are uninitialised in the encoder's workspace: columns at or past the row
//     stride are not read at all (the last head has nothing behind it) and columns >= L
//     are zeroed in registers, so LDS holds exact zeros there (P is exactly 0 for those keys;
//     0 * NaN would not be).
//   * each wave: S^T = K Q^T (v_mfma_f32_32x32x16_f16, the swapped form: lane (q = lane & 31,
//     h = lane >> 5) holds keys kb*32 + (r&3) + 8(r>>2) + 4h of its query row), the tile's row
//     max in-lane + one cross-half exchange, then m' = max(m, tile max), f = exp2((m - m') c),
//     l = l f + sum p, O = O f (every tile: no deferred rescale), P -> fp16, O^T += V^T P^T.
// LDS: 2 stages x (K [64][64] + V^T [64][68]) fp16 = 33 792 B.
constexpr int kLongWaves = 4, kLongTile = 64;
constexpr int kLongVS = vt_stride(kLongTile);                   // V^T tile row stride (2 mod 4 dwords)
constexpr int kLongStage = kLongTile * 64 + 64 * kLongVS;        // halves per stage
constexpr int kLongKPieces = kLongTile * 8 / (kLongWaves * 64);  // 16-byte K pieces per thread
constexpr int kLongVPieces = 64 * (kLongTile / 4) / (kLongWaves * 64);  // 8-byte V^T pieces per thread

__global__ __launch_bounds__(kLongWaves * 64) void mhsa_long_kernel(const _Float16* __restrict__ q,
                                                                   const _Float16* __restrict__ k,
                                                                   const _Float16* __restrict__ vt,
                                                                   _Float16* __restrict__ o, int L, int H, int stride,
                                                                   int nqc, float scale_log2) {
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * kLongStage];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hh = lane >> 5, ql = lane & 31;
    const int64_t bh = blockIdx.x / nqc;
    const int qb = (int)(blockIdx.x % nqc) * kLongWaves + wid;
    const int qi = qb * 32 + ql;
    const bool active = qb * 32 < L;  // (wave-uniform; idle waves still copy tiles)
    const _Float16* kh = k + bh * (int64_t)L * 64;
    const _Float16* vh = vt + bh * 64 * (int64_t)stride;
    const int ntiles = (L + kLongTile - 1) / kLongTile;

    f16x8 kr[kLongKPieces];  // (ext-vector types: hipcc keeps an array of the uint4 struct in scratch)
    uint2 vr[kLongVPieces];
    auto fetch = [&](int t) {
        const int k0 = t * kLongTile;
#pragma unroll
        for (int v = 0; v < kLongKPieces; v++) {
            const int e = tid + kLongWaves * 64 * v, r = e >> 3, c = e & 7;
            const int row = k0 + r < L ? k0 + r : L - 1;
            kr[v] = *(const f16x8*)(kh + (int64_t)row * 64 + c * 8);
        }
#pragma unroll
        for (int v = 0; v < kLongVPieces; v++) {
            const int e = tid + kLongWaves * 64 * v, d = e >> 4, col = k0 + 4 * (e & 15);
            // a piece that starts below L ends inside the row (col + 4 <= stride: both multiples
            // of 4, L <= stride); one at or past L re-reads the row's first piece and is zeroed
            // in stash(), so every load is unconditional and none waits for its data here
            vr[v] = *(const uint2*)(vh + (int64_t)d * stride + (col < L ? col : 0));
        }
    };
    auto stash = [&](int stage, int t) {
        _Float16* sK = lds + stage * kLongStage;
        _Float16* sV = sK + kLongTile * 64;
#pragma unroll
        for (int v = 0; v < kLongKPieces; v++) {
            const int e = tid + kLongWaves * 64 * v;
            *(f16x8*)(sK + kswz(e >> 3, e & 7)) = kr[v];
        }
#pragma unroll
        for (int v = 0; v < kLongVPieces; v++) {
            const int e = tid + kLongWaves * 64 * v;
            const int n = L - (t * kLongTile + 4 * (e & 15));  // valid halves of this piece (<= 0: none)
            uint2 w = vr[v];
            w.x &= n >= 2 ? 0xffffffffu : n == 1 ? 0x0000ffffu : 0u;
            w.y &= n >= 4 ? 0xffffffffu : n == 3 ? 0x0000ffffu : 0u;
            *(uint2*)(sV + (e >> 4) * kLongVS + 4 * (e & 15)) = w;
        }
    };

    fetch(0);
    // Q rows of this wave's queries (rows >= L read row L-1: finite, never stored), retired by
    // the explicit wait below (load_q4, attention.h): loads hipcc tracks stay pending in its
    // model around the loop's back edge, and it then waits for vmcnt(0) in front of every tile's
    // S MFMAs, which also drains the tile prefetch.
    f16x8 qf[4];
    load_q4(q + (bh * L + (qi < L ? qi : L - 1)) * 64 + hh * 8, qf);
    stash(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pin_q4(qf);
    __syncthreads();

    float m = -__builtin_inff(), l = 0.f;
    f32x16 oacc[2] = {f32x16{}, f32x16{}};
    for (int t = 0; t < ntiles; t++) {
        const bool more = t + 1 < ntiles;
        if (more) fetch(t + 1);
        if (active) {
            const _Float16* sK = lds + (t & 1) * kLongStage;
            const _Float16* sV = sK + kLongTile * 64;
            f32x16 s[2];
#pragma unroll
            for (int kb = 0; kb < 2; kb++) {
                f32x16 a = f32x16{};
#pragma unroll
                for (int ks = 0; ks < 4; ks++) {
                    const f16x8 kf = *(const f16x8*)(sK + kswz(kb * 32 + ql, 2 * ks + hh));
                    a = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], a, 0, 0, 0);
                }
                s[kb] = a;
            }
            if ((t + 1) * kLongTile > L) {  // the last tile: keys >= L
#pragma unroll
                for (int kb = 0; kb < 2; kb++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int key = t * kLongTile + kb * 32 + acc_key(r, hh);
                        s[kb][r] = key < L ? s[kb][r] : -__builtin_inff();
                    }
            }
            float mt = fmaxf(s[0][0], s[1][0]);
#pragma unroll
            for (int r = 1; r < 16; r++) mt = fmaxf(mt, fmaxf(s[0][r], s[1][r]));
            // every tile holds a key < L, so mn is finite; m = -inf (the first tile) gives f = 0
            const float mn = fmaxf(m, xhalf_max(mt));
            const float f = __builtin_amdgcn_exp2f((m - mn) * scale_log2);
            m = mn;
            const float mb = -mn * scale_log2;
            const f32x2v sc2 = {scale_log2, scale_log2}, mb2 = {mb, mb};
            f32x2v sum2 = {0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < 2; kb++)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const f32x2v a = __builtin_elementwise_fma(f32x2v{s[kb][r], s[kb][r + 1]}, sc2, mb2);
                    const f32x2v p = {__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
                    s[kb][r] = p.x;
                    s[kb][r + 1] = p.y;
                    sum2 += p;
                }
            l = l * f + (sum2.x + sum2.y);
#pragma unroll
            for (int db = 0; db < 2; db++)
#pragma unroll
                for (int r = 0; r < 16; r++) oacc[db][r] *= f;
#pragma unroll
            for (int kb = 0; kb < 2; kb++)
#pragma unroll
                for (int sp = 0; sp < 2; sp++) {
                    f16x8 pf;
#pragma unroll
                    for (int j = 0; j < 8; j++) pf[j] = (_Float16)s[kb][8 * sp + j];
#pragma unroll
                    for (int db = 0; db < 2; db++) {
                        const _Float16* vp = sV + (db * 32 + ql) * kLongVS + kb * 32 + 16 * sp + 4 * hh;
                        const f16x4 v0 = *(const f16x4*)(vp);
                        const f16x4 v1 = *(const f16x4*)(vp + 8);
                        const f16x8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[db], 0, 0, 0);
                    }
                }
        }
        // the other stage's readers finished before the previous barrier
        if (more) stash((t + 1) & 1, t + 1);
        __syncthreads();
    }
    if (active) store_o_wide(oacc, 1.0f / xhalf_sum(l), qi, hh, L, bh, H, o);
}

int mhsa_long(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H, hipStream_t s) {
    const int stride = attn_vt_stride(L);
    RM_REQUIRE(stride > 0, "mhsa_long: sequence length must be in 1..1024");
    RM_REQUIRE(nseq >= 0 && H >= 1, "mhsa_long: bad shape");
    if (nseq == 0) return OK;
    const int nqc = ((L + 31) / 32 + kLongWaves - 1) / kLongWaves;
    RM_REQUIRE(nseq * H * nqc < (1ll << 31), "mhsa_long: too many (sequence, head) pairs");
    hipLaunchKernelGGL(mhsa_long_kernel, dim3((unsigned)(nseq * H * nqc)), dim3(kLongWaves * 64), 0, s,
                       (const _Float16*)q, (const _Float16*)k, (const _Float16*)vt, (_Float16*)o, L, H, stride, nqc,
                       kAttnScaleLog2);
    RM_LAUNCHED();
    return OK;
}

// CLS query only for L <= 1024 (the last block of the inference path beyond 256 tokens): one
// wave per (sequence, head), mhsa_cls_kernel's arithmetic with the keys walked in chunks and the
// scores kept in LDS instead of per-lane arrays: lane t-strided fp32 scores, wave-reduced
// softmax, probabilities rounded to fp16 and left in LDS, lane d sums p_t * V^T[d][t] over its
// row in key order, one fp16 rounding of the output.  V^T is read in 8-byte pieces that start
// below L (so they end inside the row) and elements >= L are never used.
// q [nseq*H][64], k [nseq*H][L][64], vt [nseq*H][64][stride] -> o [nseq][H*64].
constexpr int kClsLongMax = kAttnLongMax;

__global__ __launch_bounds__(256) void mhsa_cls_long_kernel(const _Float16* __restrict__ q,
                                                            const _Float16* __restrict__ k,
                                                            const _Float16* __restrict__ vt, _Float16* __restrict__ o,
                                                            int64_t nbh, int L, int H, int stride, float scale_log2) {
    __shared__ float sp[4][kClsLongMax];
    __shared__ float sq[4][64];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t bh = (int64_t)blockIdx.x * 4 + wid;
    if (bh >= nbh) return;
    sq[wid][lane] = (float)q[bh * 64 + lane];
    __builtin_amdgcn_wave_barrier();
    const _Float16* kh = k + bh * (int64_t)L * 64;
    float mx = -__builtin_inff();
    for (int t = lane; t < L; t += 64) {
        float a = 0.f;
        const f16x8* kr = (const f16x8*)(kh + (int64_t)t * 64);
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const f16x8 kv = kr[c];
#pragma unroll
            for (int e = 0; e < 8; e++) a += sq[wid][c * 8 + e] * (float)kv[e];
        }
        a *= scale_log2;
        sp[wid][t] = a;
        mx = fmaxf(mx, a);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int t = lane; t < L; t += 64) {
        const float p = __builtin_amdgcn_exp2f(sp[wid][t] - mx);
        sp[wid][t] = (float)(_Float16)p;  // fp16-rounded, as the blocked kernels feed their P.V MFMAs
        sum += p;
    }
    sum = wave_sum(sum);
    __builtin_amdgcn_wave_barrier();
    const _Float16* vrow = vt + (bh * 64 + lane) * (int64_t)stride;
    float acc = 0.f;
    for (int c0 = 0; c0 < L; c0 += 32) {  // 8 pieces in flight per lane
        f16x4 vv[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (c0 + 4 * i < L) vv[i] = *(const f16x4*)(vrow + c0 + 4 * i);
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (c0 + 4 * i + e < L) acc += sp[wid][c0 + 4 * i + e] * (float)vv[i][e];
    }
    const int64_t b = bh / H, h = bh % H;
    o[b * (int64_t)H * 64 + h * 64 + lane] = (_Float16)(acc / sum);
}

int mhsa_cls_long(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H, hipStream_t s) {
    const int stride = attn_vt_stride(L);
    RM_REQUIRE(stride > 0, "mhsa_cls_long: sequence length must be in 1..1024");
    RM_REQUIRE(nseq >= 0 && H >= 1, "mhsa_cls_long: bad shape");
    if (nseq == 0) return OK;
    const int64_t nbh = nseq * H;
    RM_REQUIRE(nbh < (1ll << 31), "mhsa_cls_long: too many (sequence, head) pairs");
    hipLaunchKernelGGL(mhsa_cls_long_kernel, dim3(ceil_div(nbh, 4)), dim3(256), 0, s, (const _Float16*)q,
                       (const _Float16*)k, (const _Float16*)vt, (_Float16*)o, nbh, L, H, stride, kAttnScaleLog2);
    RM_LAUNCHED();
    return OK;
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_attn_vt_stride(int L) { return attn_vt_stride(L); }

REIDMI_API int reidmi_mhsa_long_f16(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L, int H,
                                     void* stream) {
    return mhsa_long(q, k, vt, o, nseq, L, H, (hipStream_t)stream);
}

#ifdef REIDMI_TOOLS
// The single-query kernel of the last block's K / V path beyond 256 tokens (run_block_cls),
// through its own launcher so tests/test_gpu_attention_long.py can compare it with fp64 and
// with query row 0 of reidmi_mhsa_long_f16 at any length.
REIDMI_API int reidmi_mhsa_cls_long_f16(const void* q, const void* k, const void* vt, void* o, int64_t nseq, int L,
                                         int H, void* stream) {
    return mhsa_cls_long(q, k, vt, o, nseq, L, H, (hipStream_t)stream);
}
#endif
