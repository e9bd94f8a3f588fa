// combine.hip — weighted, indexed combination of feature rows, optionally L2-normalised, on gfx950.
//
//   reidmi_combine_rows_f32   out[r] = f(base_w * base[r], { w[t] * src[idx[t]] : t in row r's list })
//
// The one device operation behind query expansion (AQE / alpha-QE), database augmentation and
// group pooling (evaluate.py: expand_features, database_augmentation, pool_features).  The lists
// are CSR (offsets int64 [rows + 1], idx int32, w fp32 or NULL).  The arithmetic contract is in
// include/reidmi.h; in short: one fp32 accumulator per column, entries added in list order with a
// rounded product and a rounded sum (no FMA), so a plain float32 numpy loop is the exact oracle.
//
// Kernel shape.  The work is HBM- and latency-bound (entries x d x 4 bytes read, d x 4 written):
//   * d >= 256: one 256-thread workgroup per output row; d < 256: one wave per row, four rows per
//     workgroup.  Lane t of a row owns the columns 4 (t + T u) .. + 3 of a pass (T lanes per row,
//     u < U), so a wave's 16-byte loads of one gathered row are contiguous; its accumulators stay
//     in registers.  A pass covers 4 T U columns (2048 / 256); wider rows take further passes
//     over the list.
//   * Every wave reads the row's list itself, 64 entries at a time, one entry per lane.  The kept
//     entries (0 <= idx < n_src) are a ballot mask; the wave walks its set bits in order and
//     broadcasts idx / w with v_readlane, so the gathered row's address is scalar, skipped entries
//     cost nothing, and no LDS or barrier is needed for the list.
//   * The loads of up to 8 list entries are issued before the first is consumed (8, 4, 2, 1 as the
//     mask runs out); the adds stay in list order.
//   * 16-byte loads and stores when every pointer is 16-byte aligned and d and the pitches are
//     multiples of 4; otherwise the same columns with 4-byte accesses (ld_src = d + 3 works).
//   * normalize: the squared norm is rownorm.h's single fmaf chain over the columns ascending.
//     The row is staged in LDS a pass at a time and one lane walks the chain (the waves of the
//     other resident workgroups hide it); the row is then scaled from registers (one pass) or
//     from the unnormalised values this lane wrote itself (several passes).
#include "common.h"
#include "rownorm.h"

namespace reidmi {

constexpr int CB_THREADS = 256;  // per workgroup
constexpr int CB_U_WIDE = 2;     // float4 per lane and pass, d >= 256 (2048 columns a pass)
constexpr int CB_NARROW_D = 256; // below: one wave per row
enum CombineOp : int { CB_SUM_W = 0, CB_SUM = 1, CB_MAX = 2 };

struct CbArgs {
    const float* src;
    int64_t n_src, d, ld_src;
    const int64_t* offsets;
    const int32_t* idx;
    const float* w;
    int64_t rows;
    const float* base;
    int64_t ld_base;
    float base_w;
    int mean, normalize;
    float* out;
    int64_t ldo;
    int32_t* bad;
};

// Columns c .. c + 3 of a row (c % 4 == 0); columns >= d read as +0 and are never stored.
template <bool VEC>
__device__ __forceinline__ float4 cb_load4(const float* p, int64_t c, int64_t d) {
    if constexpr (VEC) {
        return *(const float4*)(p + c);  // d % 4 == 0: c < d implies c + 3 < d
    } else {
        float4 v;
        v.x = p[c];
        v.y = c + 1 < d ? p[c + 1] : 0.0f;
        v.z = c + 2 < d ? p[c + 2] : 0.0f;
        v.w = c + 3 < d ? p[c + 3] : 0.0f;
        return v;
    }
}

template <bool VEC>
__device__ __forceinline__ void cb_store4(float* p, int64_t c, int64_t d, float4 v) {
    if constexpr (VEC) {
        *(float4*)(p + c) = v;
    } else {
        p[c] = v.x;
        if (c + 1 < d) p[c + 1] = v.y;
        if (c + 2 < d) p[c + 2] = v.z;
        if (c + 3 < d) p[c + 3] = v.w;
    }
}

template <int OP>
__device__ __forceinline__ float cb_op(float acc, float w, float v) {
    if constexpr (OP == CB_SUM_W) return __fadd_rn(acc, __fmul_rn(w, v));
    if constexpr (OP == CB_SUM) return __fadd_rn(acc, v);
    return fmaxf(acc, v);
}

template <int OP>
__device__ __forceinline__ float4 cb_op4(float4 a, float w, float4 v) {
    return make_float4(cb_op<OP>(a.x, w, v.x), cb_op<OP>(a.y, w, v.y), cb_op<OP>(a.z, w, v.z),
                       cb_op<OP>(a.w, w, v.w));
}

// Takes the next E kept entries of the wave's chunk (the lowest E set bits of m, list order):
// all E x U loads first, then the adds in list order.
template <int OP, int U, bool VEC, int E>
__device__ __forceinline__ void cb_take(uint64_t& m, int my_j, float my_w, const float* __restrict__ src,
                                        int64_t ld_src, int64_t d, const int64_t (&col)[U], float4 (&acc)[U]) {
    const float* row[E];
    float w[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int lane = __builtin_ctzll(m);
        m &= m - 1;
        row[e] = src + (int64_t)__builtin_amdgcn_readlane(my_j, lane) * ld_src;
        w[e] = OP == CB_SUM_W ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), lane)) : 1.0f;
    }
    float4 v[U][E];
#pragma unroll
    for (int u = 0; u < U; u++)
        if (col[u] < d) {
#pragma unroll
            for (int e = 0; e < E; e++) v[u][e] = cb_load4<VEC>(row[e], col[u], d);
        }
#pragma unroll
    for (int u = 0; u < U; u++)
        if (col[u] < d) {
#pragma unroll
            for (int e = 0; e < E; e++) acc[u] = cb_op4<OP>(acc[u], w[e], v[u][e]);
        }
}

// T lanes per output row (256: one row per workgroup; 64: one wave per row, four rows).
template <int OP, int T, int U, bool VEC>
__global__ __launch_bounds__(CB_THREADS) void combine_rows_kernel(const CbArgs a) {
    constexpr int RPB = CB_THREADS / T, TILE = 4 * T * U;
    __shared__ __attribute__((aligned(16))) float s_row[RPB][TILE];
    __shared__ float s_ss[RPB];
    const int sub = threadIdx.x / T, t = threadIdx.x % T, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * RPB + sub;
    const bool live = r < a.rows;  // uniform per wave; dead waves only keep the barriers company
    const int64_t d = a.d;
    int64_t o0 = 0, len = 0;
    if (live) {
        o0 = a.offsets[r];
        len = a.offsets[r + 1] - o0;
        if (len < 0) len = 0;
    }
    const float* brow = a.base && live ? a.base + r * a.ld_base : nullptr;
    float* orow = live ? a.out + r * a.ldo : nullptr;
    float ss = 0.0f;  // the squared-norm chain (lane t == 0 of the row)
    float4 acc[U];
    float cnt_f = 1.0f;

    for (int64_t c0 = 0; c0 < d; c0 += TILE) {  // uniform over the workgroup
        int64_t col[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            col[u] = c0 + 4 * (t + T * u);
            acc[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        if (live) {
            bool have = brow != nullptr;  // max: whether acc holds a row yet
            if (brow) {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (col[u] < d) {
                        const float4 b = cb_load4<VEC>(brow, col[u], d);
                        acc[u] = OP == CB_MAX ? b
                                              : make_float4(__fmul_rn(a.base_w, b.x), __fmul_rn(a.base_w, b.y),
                                                            __fmul_rn(a.base_w, b.z), __fmul_rn(a.base_w, b.w));
                    }
            }
            int64_t kept = 0;
            for (int64_t cs = 0; cs < len; cs += 64) {
                const int64_t e = cs + lane;
                int my_j = -1;
                float my_w = 1.0f;
                if (e < len) {
                    my_j = a.idx[o0 + e];
                    if (OP == CB_SUM_W) my_w = a.w[o0 + e];
                }
                uint64_t m = __ballot(my_j >= 0 && (int64_t)my_j < a.n_src);
                if (a.bad != nullptr && c0 == 0 && t < 64) {  // once per row: its first wave, first pass
                    const uint64_t over = __ballot(my_j >= 0 && (int64_t)my_j >= a.n_src);
                    if (over != 0 && lane == 0) atomicAdd(a.bad, (int32_t)__builtin_popcountll(over));
                }
                kept += __builtin_popcountll(m);
                if (OP == CB_MAX && !have && m != 0) {  // the first kept row starts the maximum
                    const int l0 = __builtin_ctzll(m);
                    m &= m - 1;
                    const float* row = a.src + (int64_t)__builtin_amdgcn_readlane(my_j, l0) * a.ld_src;
#pragma unroll
                    for (int u = 0; u < U; u++)
                        if (col[u] < d) acc[u] = cb_load4<VEC>(row, col[u], d);
                    have = true;
                }
                while (__builtin_popcountll(m) >= 8) cb_take<OP, U, VEC, 8>(m, my_j, my_w, a.src, a.ld_src, d, col, acc);
                if (__builtin_popcountll(m) >= 4) cb_take<OP, U, VEC, 4>(m, my_j, my_w, a.src, a.ld_src, d, col, acc);
                if (__builtin_popcountll(m) >= 2) cb_take<OP, U, VEC, 2>(m, my_j, my_w, a.src, a.ld_src, d, col, acc);
                if (m != 0) cb_take<OP, U, VEC, 1>(m, my_j, my_w, a.src, a.ld_src, d, col, acc);
            }
            if (a.mean) {
                const int64_t n = kept + (brow ? 1 : 0);
                cnt_f = n > 0 ? (float)n : 1.0f;  // nothing kept, no base: the row stays +0
#pragma unroll
                for (int u = 0; u < U; u++)
                    acc[u] = make_float4(__fdiv_rn(acc[u].x, cnt_f), __fdiv_rn(acc[u].y, cnt_f),
                                         __fdiv_rn(acc[u].z, cnt_f), __fdiv_rn(acc[u].w, cnt_f));
            }
            // several passes: the unnormalised values go out now (each lane reads its own back)
            if (!a.normalize || d > TILE) {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (col[u] < d) cb_store4<VEC>(orow, col[u], d, acc[u]);
            }
        }
        if (a.normalize) {  // uniform
            if (live) {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (col[u] < d) *(float4*)&s_row[sub][4 * (t + T * u)] = acc[u];
            }
            __syncthreads();
            if (live && t == 0) {
                const int n = (int)(d - c0 < TILE ? d - c0 : TILE);
                for (int k = 0; k < n; k++) ss = l2_sq_step(ss, s_row[sub][k]);
            }
            __syncthreads();
        }
    }
    if (!a.normalize) return;
    if (live && t == 0) s_ss[sub] = ss;
    __syncthreads();
    if (!live) return;
    const float den = l2_denominator(s_ss[sub]);
    for (int64_t c0 = 0; c0 < d; c0 += TILE) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t c = c0 + 4 * (t + T * u);
            if (c < d) {
                const float4 v = d > TILE ? cb_load4<VEC>(orow, c, d) : acc[u];
                cb_store4<VEC>(orow, c, d,
                               make_float4(l2_scale(v.x, den), l2_scale(v.y, den), l2_scale(v.z, den),
                                           l2_scale(v.w, den)));
            }
        }
    }
}

template <int OP, bool VEC>
static void combine_launch(const CbArgs& a, hipStream_t s) {
    if (a.d >= CB_NARROW_D) {
        hipLaunchKernelGGL((combine_rows_kernel<OP, CB_THREADS, CB_U_WIDE, VEC>), dim3((unsigned)a.rows),
                           dim3(CB_THREADS), 0, s, a);
    } else {
        hipLaunchKernelGGL((combine_rows_kernel<OP, 64, 1, VEC>), dim3((unsigned)ceil_div(a.rows, CB_THREADS / 64)),
                           dim3(CB_THREADS), 0, s, a);
    }
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_combine_rows_f32(const float* src, int64_t n_src, int64_t d, int64_t ld_src,
                                       const int64_t* offsets, const int32_t* idx, const float* w, int64_t rows,
                                       const float* base, int64_t ld_base, float base_w, int mode, int normalize,
                                       float* out, int64_t ldo, int32_t* bad, void* stream) {
    RM_REQUIRE(rows >= 0 && rows < ((int64_t)1 << 31), "combine_rows: rows must be in [0, 2^31)");
    RM_REQUIRE(mode >= 0 && mode <= 2, "combine_rows: mode must be 0 (sum), 1 (mean) or 2 (max)");
    RM_REQUIRE(d > 0, "combine_rows: d must be positive");
    RM_REQUIRE(ld_src >= d && ldo >= d, "combine_rows: ld_src and ldo must be at least d");
    RM_REQUIRE(base == nullptr || ld_base >= d, "combine_rows: ld_base must be at least d");
    RM_REQUIRE(n_src >= 0 && n_src < ((int64_t)1 << 31), "combine_rows: n_src must be in [0, 2^31) (int32 indices)");
    RM_REQUIRE(mode != 2 || w == nullptr, "combine_rows: max takes no weights");
    if (rows == 0) return OK;
    RM_REQUIRE(src != nullptr && offsets != nullptr && idx != nullptr && out != nullptr,
               "combine_rows: src, offsets, idx and out must not be null");
    CbArgs a{src, n_src, d, ld_src, offsets, idx, w, rows, base, ld_base, base_w, mode == 1, normalize != 0,
             out, ldo, bad};
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const bool vec = d % 4 == 0 && ld_src % 4 == 0 && ldo % 4 == 0 && al16(src) && al16(out) &&
                     (base == nullptr || (ld_base % 4 == 0 && al16(base)));
    hipStream_t s = (hipStream_t)stream;
    const int op = mode == 2 ? CB_MAX : (w != nullptr ? CB_SUM_W : CB_SUM);
    if (op == CB_SUM_W) vec ? combine_launch<CB_SUM_W, true>(a, s) : combine_launch<CB_SUM_W, false>(a, s);
    else if (op == CB_SUM) vec ? combine_launch<CB_SUM, true>(a, s) : combine_launch<CB_SUM, false>(a, s);
    else vec ? combine_launch<CB_MAX, true>(a, s) : combine_launch<CB_MAX, false>(a, s);
    RM_LAUNCHED();
    return OK;
}
