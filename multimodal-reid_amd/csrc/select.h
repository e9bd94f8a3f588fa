// select.h — the (value, index) selection helpers of the retrieval kernels: the stable-argsort
// key order, the in-LDS bitonic sort and the streaming K-smallest selection of one row
// (evaluate.py:40, reranking.py:48: the first k of np.argsort(row)).  Device-only, internal;
// the one definition for search.hip, prefilter.hip and eval.hip.
#pragma once
#include "common.h"

namespace reidmi {

// ---------------------------------------------------------------- key helpers
__device__ __forceinline__ bool key_less(float av, int ai, float bv, int bi) {
    return av < bv || (av == bv && ai < bi);
}

// In-LDS bitonic sort of (v,i) pairs, ascending by (v, i); P a power of two.
__device__ inline void bitonic_sort_kv(float* sv, int* si, int P) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P; t += blockDim.x) {
                int o = t ^ j;
                if (o > t) {
                    bool up = (t & k) == 0;
                    float av = sv[t], bv = sv[o];
                    int ai = si[t], bi = si[o];
                    bool gt = key_less(bv, bi, av, ai);
                    if (gt == up) { sv[t] = bv; sv[o] = av; si[t] = bi; si[o] = ai; }
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int pow2_ceil(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// --------------------------------------------------------------------- top-k
// Per row: k smallest (value, index) pairs in ascending order == np.argsort(kind="stable")[:k].
// Streams the row once; a candidate buffer in LDS collects elements under the running
// k-th key and is merged (bitonic) into the selection when it fills.
constexpr int TK_CAP = 2048, TK_CHUNK = 1024;

struct TkLds {
    float sv[TK_CAP];
    int si[TK_CAP];
    int s_cnt, s_nsel;
    float s_tv;
    int s_ti;
};

// The selection of one row by the whole workgroup: afterwards L.sv / L.si [0, min(K, cols))
// hold the K smallest (val(j), idx(j)) in ascending (value, index) order among the j with
// keep(v, idx(j)).  idx(j) is the index the order and the result carry: the position j itself
// (the default) or what position j of a list stands for; it must be unique among the kept j.
// K <= TK_CAP - TK_CHUNK.
struct KeepAll {
    __device__ bool operator()(float, int) const { return true; }
};
struct IdxIsPos {
    __device__ int operator()(int64_t j) const { return (int)j; }
};
template <typename VAL, typename KEEP = KeepAll, typename IDX = IdxIsPos>
__device__ inline void topk_row_dev(VAL val, int64_t cols, int K, TkLds& L, KEEP keep = KEEP{}, IDX idx = IDX{}) {
    if (threadIdx.x == 0) { L.s_cnt = 0; L.s_nsel = 0; L.s_tv = __builtin_inff(); L.s_ti = 0x7fffffff; }
    __syncthreads();
    for (int64_t c0 = 0; c0 < cols; c0 += TK_CHUNK) {
        const float tv = L.s_tv;
        const int ti = L.s_ti, nsel = L.s_nsel;
#pragma unroll
        for (int u = 0; u < TK_CHUNK / 256; u++) {
            int64_t j = c0 + u * 256 + threadIdx.x;
            if (j < cols) {
                const float v = val(j);
                const int ji = idx(j);
                if (key_less(v, ji, tv, ti) && keep(v, ji)) {
                    int p = atomicAdd(&L.s_cnt, 1);
                    L.sv[nsel + p] = v;
                    L.si[nsel + p] = ji;
                }
            }
        }
        __syncthreads();
        const bool last = c0 + TK_CHUNK >= cols;
        const int n = L.s_nsel + L.s_cnt;
        __syncthreads();  // every thread has read s_cnt before anyone appends again
        if (last || n > TK_CAP - TK_CHUNK) {
            const int P = pow2_ceil(n < 2 ? 2 : n);
            for (int t = n + threadIdx.x; t < P; t += blockDim.x) { L.sv[t] = __builtin_inff(); L.si[t] = 0x7fffffff; }
            __syncthreads();
            bitonic_sort_kv(L.sv, L.si, P);
            if (threadIdx.x == 0) {
                int ns = n < K ? n : K;
                L.s_nsel = ns;
                L.s_cnt = 0;
                if (ns == K) { L.s_tv = L.sv[K - 1]; L.s_ti = L.si[K - 1]; }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------- partial lists
// A partial list entry is a float2 (value, the index's bits); padding is (+inf, -1).
__device__ __forceinline__ int kv_idx(float2 e) { return __float_as_int(e.y); }

// Joins the partial lists of one row by the whole workgroup: at(p), p < total, is entry p of
// their concatenation, (value, the index it stands for); an entry with a negative index is
// padding and is skipped.  The order is key_less on (value, that index), whatever the order of
// the lists and of the entries inside them; the caller guarantees that no index occurs twice.
// (Lists sorted by (value, index) over ascending index ranges, the fused kernels' own, come out
// as they did under the order by position: the two orders agree there.)  out_idx / out_dist
// (nullable) [K] get the K smallest, a short result padded with -1 / +inf; they are written
// after the last at().
template <typename AT>
__device__ inline void topk_merge_dev(AT at, int64_t total, int K, TkLds& L, int32_t* __restrict__ out_idx,
                                      float* __restrict__ out_dist) {
    topk_row_dev([&](int64_t p) { return at(p).x; }, total, K, L, [](float, int i) { return i >= 0; },
                 [&](int64_t p) { return kv_idx(at(p)); });
    const int n = L.s_nsel;
    for (int t = threadIdx.x; t < K; t += blockDim.x) {
        out_idx[t] = t < n ? L.si[t] : -1;
        if (out_dist) out_dist[t] = t < n ? L.sv[t] : __builtin_inff();
    }
}

}  // namespace reidmi
