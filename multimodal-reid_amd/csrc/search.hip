// search.hip — ranked matches of the CLIP-ReID eval path on gfx950: row top-k and the fused search.
//
//   reidmi_topk_rows_f32   first k of np.argsort(row) (stable)          evaluate.py:40, reranking.py:48
//   reidmi_search_f32      the k nearest gallery rows per query, with   evaluate.py:7-13, 40, 46-48
//                          eval_func's same-id same-camera removal,
//                          without the Q x G matrix
//   reidmi_search_bounded_f32  the same under a per-query bound (a radius, or the k-th key of a
//                          list carried from earlier gallery blocks): the bound is the initial
//                          threshold of the row, so the epilogue filters against it from tile one
//   reidmi_search_filtered_f32  the same over the items a filter admits (admit.h: validity, camera
//                          mask, time window and group clauses next to the label rule)
//
// The distance tile is distance.h's (the distance kernels' bits), the selection select.h's.
#include "admit.h"
#include "backend.h"
#include "distance.h"
#include "select.h"

namespace reidmi {

// --------------------------------------------------------------------- top-k rows
// topk_row_dev (select.h) per row of a matrix.  Optional per-row divisor implements
// reranking.py:46 (od[i,:] = D[i,:] / colmax[i] for symmetric D).
// K > TK_RUN (reranking.py:48's initial_rank for k1 or k2 beyond 1023): rounds of TK_RUN, each
// a fresh stream over the row keeping only the keys after the last one selected (keys are
// unique: the index breaks every tie), so the rounds concatenate to the stable argsort prefix.
constexpr int TK_RUN = TK_CAP - TK_CHUNK;

__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ x, int64_t cols, int64_t ld,
                                                        const float* __restrict__ row_div, int K,
                                                        int32_t* __restrict__ out_idx, float* __restrict__ out_val,
                                                        int64_t ldo) {
    __shared__ TkLds L;
    const int64_t row = blockIdx.x;
    const float* base = x + row * ld;
    const bool has_div = row_div != nullptr;
    const float dv = has_div ? row_div[row] : 1.0f;
    auto val = [&](int64_t j) {
        float v = base[j];
        if (has_div) v = v / dv;
        return v;
    };
    float lv = -__builtin_inff();
    int li = -1;
    for (int done = 0; done < K;) {
        const int kk = K - done < TK_RUN ? K - done : TK_RUN;
        if (done == 0)
            topk_row_dev(val, cols, kk, L);
        else
            topk_row_dev(val, cols, kk, L, [&](float v, int j) { return key_less(lv, li, v, j); });
        for (int r = threadIdx.x; r < kk; r += blockDim.x) {
            out_idx[row * ldo + done + r] = L.si[r];
            if (out_val) out_val[row * ldo + done + r] = L.sv[r];
        }
        lv = L.sv[kk - 1];
        li = L.si[kk - 1];
        done += kk;
        __syncthreads();  // every thread has read the selection before the next round refills it
    }
}

int topk_launch(const float* x, int64_t rows, int64_t cols, int64_t ldx, const float* row_div, int K,
                int32_t* out_idx, float* out_val, int64_t ldo, hipStream_t s) {
    RM_REQUIRE(rows >= 0 && cols > 0 && ldx >= cols && K > 0 && K <= cols && ldo >= K,
               "topk_rows: need 0 < k <= cols, ldo >= k");
    RM_REQUIRE(cols < 0x7fffffff, "topk_rows: cols must fit int32");
    if (rows == 0) return OK;
    hipLaunchKernelGGL(topk_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, x, cols, ldx, row_div, K, out_idx,
                       out_val, ldo);
    RM_LAUNCHED();
    return OK;
}

// ------------------------------------------------------------- fused top-k search
// reidmi_search_f32: the k nearest gallery rows of every query row without the Q x G matrix.
// distance.h's band-and-range walk: a workgroup owns one 128-row query band and one contiguous
// gallery range [c0, c1) and walks it in 128-column tiles with the distance kernels' mainloops
// (PIPE: a copy of dm_tile_pipe, else dm_tile_single, whose K-step is the distance kernels'
// dm_kstep) and their v = dm_value, so v below has the distance kernel's bits, and selects in
// the epilogue instead of storing:
//   * (v, j) is kept when key_less(v, j, thr[row]) and j is admitted (admit.h sr_admit: the label
//     rule and, in the FILTER instantiations, the filter's clauses; a column with g_valid == 0 is
//     skipped before the compare, the other clauses' query side is read from global memory behind
//     it, so the filtered kernel keeps the LDS below and four workgroups per CU); thr[row]
//     is the row's bound (none: +inf) until K candidates were seen, then its current K-th key, in
//     LDS, and only falls; s_own says which of the two it is (a bounded row that collects K
//     candidates must still compact once, so that its own K-th key replaces the bound; one with
//     fewer keeps the bound to the end and its final compaction pads);
//   * kept pairs are appended to the row's list of `cap` entries in the workspace (L2-resident:
//     after the first tiles a row keeps about K / t of tile t's 128 columns);
//   * between tiles a wave compacts those of its 32 rows that just reached K candidates or could
//     overflow in the next tile (count + 128 > cap): rank by counting in LDS (keys are unique:
//     the index breaks every tie), the K smallest written back in order, thr lowered.
// No other workgroup touches the band's lists of this range, so there are no races between
// workgroups.  After the last tile every row is compacted once more: list[0, K) is the range's
// sorted partial result, padded with (+inf, -1).  search_merge_kernel joins the S partial lists
// of a row.  LDS: 33 024 B of operand stages (reused as the compaction scratch, 4 waves x cap
// x 8 B) + 2.5 KB of row state (+ 2 KB of query labels): four workgroups per CU, as the distance
// kernel.
constexpr int SR_K_MAX = 128, SR_CAP_MAX = 512 /* 4 waves x 512 x 8 B of scratch fit the stages */;
static_assert(DM_SMEM >= 4 * SR_CAP_MAX * 2, "search: the compaction scratch fits the stages");

// reidmi_search_bounded_f32's per-query bound: (dist[i * ld], idx[i * ld]), the index in the space
// where this gallery's item j is base + j.  dist == nullptr: no bound; idx == nullptr: the
// inclusive radius form.  Read once, in the kernel's prologue.
struct SrBound {
    const float* dist;
    const int32_t* idx;
    int64_t ld, base;
};

// One wave compacts one row: list[0, n) -> the min(n, K) smallest in ascending (v, j) order.
__device__ __forceinline__ void sr_compact_row(float2* __restrict__ list, uint64_t* sc, int n, int K, bool last,
                                               float* tv, int* ti, int* own, int* cnt, int lane) {
    // (v, j) as one unsigned 64-bit key in key_less order: the order-preserving image of v's bits
    // above j (v is never -0: it is a sum with qq + gg >= +0; NaN never passes the filter)
    for (int t = lane; t < n; t += 64) {
        const float2 e = list[t];
        uint32_t u = __float_as_uint(e.x);
        u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
        sc[t] = ((uint64_t)u << 32) | (uint32_t)kv_idx(e);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < n; t += 64) {
        const uint64_t me = sc[t];
        int rank = 0;
        for (int u = 0; u < n; u++) rank += sc[u] < me ? 1 : 0;
        if (rank < K) {
            const uint32_t u = (uint32_t)(me >> 32);
            const float v = __uint_as_float((u >> 31) ? u ^ 0x80000000u : ~u);
            list[rank] = make_float2(v, __int_as_float((int)(uint32_t)me));
            if (rank == K - 1) { *tv = v; *ti = (int)(uint32_t)me; }
        }
    }
    const int ns = n < K ? n : K;
    if (last)
        for (int t = ns + lane; t < K; t += 64) list[t] = make_float2(__builtin_inff(), __int_as_float(-1));
    if (lane == 0) {
        *cnt = ns;
        if (n >= K) *own = 1;  // rank K - 1 existed: (tv, ti) is now the row's own K-th key
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();  // the scratch is free for the wave's next row
}

template <bool PIPE, bool LABELS, bool FILTER>
__global__ __launch_bounds__(256, DM2_MINWG) void search_f32_kernel(
    const float* __restrict__ q, const float* __restrict__ g, const float* __restrict__ qq,
    const float* __restrict__ gg, int64_t Q, int64_t G, int64_t D, int64_t ldq, int64_t ldg, int K,
    std::conditional_t<FILTER, SrFilter, SrLabels> flt, SrBound bnd, int64_t range_len, int cap, float2* __restrict__ lists, int32_t* __restrict__ stats) {
    __shared__ float smem[DM_SMEM];
    __shared__ float s_tv[DM_BM], s_qq[DM_BM];
    __shared__ int s_ti[DM_BM], s_cnt[DM_BM], s_own[DM_BM];
    __shared__ int64_t s_qp[LABELS ? DM_BM : 1], s_qc[LABELS ? DM_BM : 1];
    const DmThread t = dm_thread();
    const int tid = t.tid, lane = t.lane, wid = t.wid, wm = t.wm, wn = t.wn;
    const DmWalk w = dm_walk(Q, G, range_len);
    const int64_t bm = w.bm, c0 = w.c0, c1 = w.c1;
    float2* const mylists = lists + (w.split * w.bands + w.band) * DM_BM * (int64_t)cap;
    if (tid < DM_BM) {
        const bool in = bm + tid < Q;
        // The row's running threshold starts at its bound (none: (+inf, every index)), so the
        // epilogue's compare filters against it from the first tile on.  The bound's index moves to
        // this gallery's local j once, here: <= 0 says no local j ties in, > G (clamped to G, which
        // no j reaches) that every tie is in, as in the radius form.  Whether the threshold is the
        // row's own K-th key is s_own, not a value of s_ti.
        float tv0 = __builtin_inff();
        int ti0 = 0x7fffffff;
        if (bnd.dist != nullptr && in) {
            tv0 = bnd.dist[(bm + tid) * bnd.ld];
            if (bnd.idx != nullptr) {
                const int64_t l = (int64_t)bnd.idx[(bm + tid) * bnd.ld] - bnd.base;
                ti0 = l <= 0 ? 0 : (l > G ? (int)G : (int)l);
            }
        }
        s_tv[tid] = tv0;
        s_ti[tid] = ti0;
        s_own[tid] = 0;
        s_cnt[tid] = 0;
        s_qq[tid] = in ? qq[bm + tid] : 0.0f;
        if constexpr (LABELS) {
            s_qp[tid] = in ? flt.qp[bm + tid] : 0;
            s_qc[tid] = in ? flt.qc[bm + tid] : 0;
        }
    }
    __syncthreads();
    int kept = 0, compactions = 0;
    for (int64_t bn = c0;; bn += DM_BN) {
        if (bn < c1) {
            f32x16 acc[2][2];
            dm_acc_zero(acc);
            // the stages are carved out of smem (the compaction scratch between tiles); gallery rows end at c1
            if constexpr (PIPE) {
                // a copy of dm_tile_pipe (see there); gallery rows end at c1
                float(*sA)[DM2_BK][DM2_LD] = (float(*)[DM2_BK][DM2_LD])smem;
                float(*sB)[DM2_BK][DM2_LD] = (float(*)[DM2_BK][DM2_LD])(smem + 2 * DM2_BK * DM2_LD);
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
                    vb[u] = bn + srow[u] < c1;
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
#pragma unroll
                    for (int s = 0; s < DM2_BK / 2; s++) {
                        const int kr = 2 * s + (lane >> 5);
                        const float a0 = sA[cur][kr][wm * 64 + (lane & 31)];
                        const float a1 = sA[cur][kr][wm * 64 + 32 + (lane & 31)];
                        const float b0 = sB[cur][kr][wn * 64 + (lane & 31)];
                        const float b1 = sB[cur][kr][wn * 64 + 32 + (lane & 31)];
                        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
                    }
                    if (kt + 1 < nk) lstore(cur ^ 1);
                    __syncthreads();
                }
            } else {
                dm_tile<false>(t, q, g, Q, c1, D, ldq, ldg, bm, bn, smem, acc);
            }
            // epilogue: the distance kernels' v, filtered against the row's threshold.  il and j are
            // dm_lane_row / dm_lane_col written out: through the functions the kernel spills 8 B more per lane
#pragma unroll
            for (int nt = 0; nt < 2; nt++) {
                const int64_t j = bn + wn * 64 + nt * 32 + (lane & 31);
                if (j >= c1) continue;
                if constexpr (FILTER)
                    if (!sr_item_valid(flt, j)) continue;  // the cheapest clause: the column's 32 rows at once
                const float ggj = gg[j];
                SrItem item = {0, 0, 0, 0, 0, true};  // the gallery side, read once per column and lane
                bool lab_loaded = false;
#pragma unroll
                for (int mt = 0; mt < 2; mt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int il = wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        if (bm + il >= Q) continue;
                        const float v = dm_value(acc[mt][nt][r], s_qq[il], ggj);
                        const float tv = s_tv[il];
                        if (!(v <= tv)) continue;
                        if (!key_less(v, (int)j, tv, s_ti[il])) continue;
                        if constexpr (LABELS || FILTER) {
                            if (!lab_loaded) { item = sr_item(flt, LABELS, FILTER, j); lab_loaded = true; }
                            // the query side: the labels from LDS, the clauses' values from global
                            // memory (L2: this is the rare path after the first tiles)
                            SrRowRef row = {s_qp[LABELS ? il : 0], s_qc[LABELS ? il : 0], 0, 0, 0, 0};
                            if constexpr (FILTER) sr_row_clauses(flt, bm + il, row);
                            if (!sr_admit(flt, LABELS, FILTER, row, item)) continue;
                        }
                        const int p = atomicAdd(&s_cnt[il], 1);  // < cap: count + 128 <= cap before the tile
                        mylists[(int64_t)il * cap + p] = make_float2(v, __int_as_float((int)j));
                        kept++;
                    }
            }
        }
        __syncthreads();  // the tile's appends (LDS counts, lists) are visible; the stages are free
        const bool last = bn + DM_BN >= c1;
        {
            const int row = wid + 4 * (lane & 31);
            const int n = s_cnt[row];
            const bool over = n + DM_BN > cap;
            const bool has_thr = s_own[row] != 0;  // a carried-in bound is a threshold, but not the row's own
            const bool need = lane < 32 && bm + row < Q && (last || over || (!has_thr && n >= K));
            if (need && over && has_thr && !last) compactions++;  // stats[0]: forced by a full list
            uint64_t m = __ballot(need);
            uint64_t* sc = (uint64_t*)smem + wid * cap;
            while (m) {
                const int b = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const int rw = wid + 4 * b;
                sr_compact_row(mylists + (int64_t)rw * cap, sc, s_cnt[rw], K, last, &s_tv[rw], &s_ti[rw], &s_own[rw],
                               &s_cnt[rw], lane);
            }
        }
        __syncthreads();  // thresholds and counts of the next tile; the scratch is a stage again
        if (last) break;
    }
    if (stats) {
        if (compactions) atomicAdd(&stats[0], compactions);
        if (kept) atomicAdd(&stats[1], kept);
    }
}

// Joins the S partial lists of one row (entries carry the gallery index j: select.h
// topk_merge_dev).
__global__ __launch_bounds__(256) void search_merge_kernel(const float2* __restrict__ lists, int64_t bands, int S,
                                                           int cap, int K, int32_t* __restrict__ out_idx,
                                                           float* __restrict__ out_dist, int64_t ldo) {
    __shared__ TkLds L;
    const int64_t row = blockIdx.x, band = row / DM_BM, r = row % DM_BM;
    auto at = [&](int64_t p) { return lists[(((p / K) * bands + band) * DM_BM + r) * (int64_t)cap + p % K]; };
    topk_merge_dev(at, (int64_t)S * K, K, L, out_idx + row * ldo, out_dist ? out_dist + row * ldo : nullptr);
}

// reidmi_search_merge_f32: the same join over the rows reidmi_search_f32 writes (index and
// distance arrays, list s of row i at s * list_stride + i * ldi), an entry's index moved by its
// list's base to the global one.  One workgroup per query row, as search_merge_kernel: the S * k_in
// entries are read once, coalesced, into TkLds and sorted there (DESIGN.md §5 on the choice).
__global__ __launch_bounds__(256) void search_merge_lists_kernel(const int32_t* __restrict__ in_idx,
                                                                 const float* __restrict__ in_dist, int S, int k_in,
                                                                 int64_t list_stride, int64_t ldi,
                                                                 const int64_t* __restrict__ base, int K,
                                                                 int32_t* __restrict__ out_idx,
                                                                 float* __restrict__ out_dist, int64_t ldo) {
    __shared__ TkLds L;
    const int64_t row = blockIdx.x;
    auto at = [&](int64_t p) {
        const int s = (int)p / k_in, e = (int)p - s * k_in;  // S * k_in < 2^31
        const int64_t o = s * list_stride + row * ldi + e;
        const int j = in_idx[o];
        const int gj = j < 0 ? -1 : (int)((base ? base[s] : 0) + j);
        return make_float2(in_dist[o], __int_as_float(gj));
    };
    topk_merge_dev(at, (int64_t)S * k_in, K, L, out_idx + row * ldo, out_dist ? out_dist + row * ldo : nullptr);
}

int search_merge_launch(const int32_t* in_idx, const float* in_dist, int S, int64_t Q, int k_in, int64_t list_stride,
                        int64_t ldi, const int64_t* base, int k, int32_t* out_idx, float* out_dist, int64_t ldo,
                        void* stream) {
    RM_REQUIRE(k >= 1 && k <= SR_K_MAX, "search_merge: need 1 <= k <= 128");
    RM_REQUIRE(k_in >= 1 && k_in <= SR_K_MAX, "search_merge: need 1 <= k_in <= 128");
    RM_REQUIRE(S >= 1 && (int64_t)S * k_in < (1ll << 31), "search_merge: need S >= 1, S * k_in < 2^31");
    RM_REQUIRE(Q >= 0 && Q < (1ll << 31), "search_merge: bad Q");
    RM_REQUIRE(ldi >= k_in, "search_merge: ldi >= k_in");
    RM_REQUIRE(ldo >= k, "search_merge: ldo >= k");
    RM_REQUIRE(S == 1 || list_stride >= Q * ldi, "search_merge: list_stride >= Q * ldi (the lists overlap)");
    RM_REQUIRE(in_idx != nullptr && in_dist != nullptr, "search_merge: in_idx and in_dist required");
    RM_REQUIRE(out_idx != nullptr, "search_merge: out_idx required");
    if (Q == 0) return OK;
    hipLaunchKernelGGL(search_merge_lists_kernel, dim3((unsigned)Q), dim3(256), 0, (hipStream_t)stream, in_idx,
                       in_dist, S, k_in, list_stride, ldi, base, k, out_idx, out_dist, ldo);
    RM_LAUNCHED();
    return OK;
}

// The launcher's choices, pure functions of the arguments: distance.h's dm_walk_plan; a forced S
// (tools) cuts G into ceil(G / S) columns per range, tile-aligned or not.
struct SrPlan {
    int64_t bands, S, range_len;
    int cap;
};
static bool sr_plan(int64_t Q, int64_t G, int k, int splits, int cap, SrPlan* p) {
    if (Q < 0 || G <= 0 || G >= 0x7fffffff || k < 1 || k > SR_K_MAX || k > G) return false;
    p->bands = (Q + DM_BM - 1) / DM_BM;
    const int64_t tiles = (G + DM_BN - 1) / DM_BN;
    if (splits == 0) {
        dm_walk_plan(p->bands, tiles, &p->S, &p->range_len);
    } else {
        if (splits < 1 || splits > 4096 || splits > G) return false;
        p->S = splits;
        p->range_len = (G + splits - 1) / splits;
    }
    if (cap == 0) cap = k <= 64 ? 256 : 384;  // a full list needs 192+ (256+) new candidates past k
    if (cap < k + DM_BN || cap > SR_CAP_MAX) return false;
    p->cap = cap;
    return p->S * k < (1ll << 31) && p->bands * p->S < (1ll << 31);
}
// workspace: norms | the lists
static int64_t sr_ws_bytes(int64_t Q, int64_t G, const SrPlan& p) {
    return dm_norm_bytes(Q, G) + p.bands * p.S * DM_BM * p.cap * 8;
}

int search_impl(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D, int k,
                const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                const reidmi_search_filter* filter, const float* bound_dist, const int32_t* bound_idx, int64_t ldb,
                int64_t index_base, int32_t* out_idx, float* out_dist, int64_t ldo, void* ws, int64_t ws_bytes,
                int splits, int cap, int32_t* stats, void* stream) {
    RM_REQUIRE(Q >= 0 && G > 0 && G < 0x7fffffff && D > 0 && ldq >= D && ldg >= D, "search: bad shape");
    RM_REQUIRE(k >= 1 && k <= G, "search: need 1 <= k <= G");
    RM_REQUIRE(k <= SR_K_MAX,
               "search: k > 128 is not fused; use reidmi_distmat_f32 + reidmi_topk_rows_f32 for larger k");
    RM_REQUIRE(out_idx != nullptr && ldo >= k, "search: out_idx required, ldo >= k");
    SrFilter flt;
    RM_TRY(sr_filter_make(q_pids, q_cams, g_pids, g_cams, filter, &flt));
    RM_REQUIRE(bound_dist != nullptr || bound_idx == nullptr, "search: bound_idx needs bound_dist");
    RM_REQUIRE(ldb >= 1, "search: need ldb >= 1");
    RM_REQUIRE(index_base >= 0 && index_base + G <= 0x7fffffff,
               "search: need index_base >= 0 and index_base + G <= 2^31 - 1");
    SrPlan p;
    RM_REQUIRE(sr_plan(Q, G, k, splits, cap, &p), "search: bad splits or list capacity (k + 128 <= cap <= 512)");
    RM_REQUIRE(ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= sr_ws_bytes(Q, G, p),
               "search: workspace (reidmi_search_workspace_bytes, 16-byte aligned) required");
    if (Q == 0) return OK;
    RM_REQUIRE(q != nullptr && g != nullptr, "search: features required");
    hipStream_t s = (hipStream_t)stream;
    float* qq = (float*)ws;
    float* gg = qq + Q;
    float2* lists = (float2*)((char*)ws + dm_norm_bytes(Q, G));
    RM_TRY(dm_norms(q, Q, ldq, g, G, ldg, D, qq, gg, s));
    const SrBound bnd{bound_dist, bound_idx, ldb, index_base};
    const SrLabels lab{flt.qp, flt.qc, flt.gp, flt.gc};
    const dim3 grid((unsigned)(p.bands * p.S));
    auto arg = [&](auto filter) {
        if constexpr (decltype(filter)::value) return flt; else return lab;
    };
    // no clause present: the instantiations, and so the kernels, of the search without a filter
    RM_BOOL_SWITCH(
        dm2_ok(q, ldq, g, ldg, D), PIPE,
        RM_BOOL_SWITCH(flt.qp != nullptr, LABELS,
                       RM_BOOL_SWITCH(sr_has_clauses(flt), FILTER,
                                      hipLaunchKernelGGL((search_f32_kernel<PIPE, LABELS, FILTER>), grid, dim3(256), 0,
                                                         s, q, g, qq, gg, Q, G, D, ldq, ldg, k,
                                                         arg(std::bool_constant<FILTER>{}), bnd, p.range_len,
                                                         p.cap, lists, stats))));
    RM_LAUNCHED();
    hipLaunchKernelGGL(search_merge_kernel, dim3((unsigned)Q), dim3(256), 0, s, (const float2*)lists, p.bands,
                       (int)p.S, p.cap, k, out_idx, out_dist, ldo);
    RM_LAUNCHED();
    return OK;
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_topk_rows_f32(const float* x, int64_t rows, int64_t cols, int64_t ldx, const float* row_div,
                                    int k, int32_t* out_idx, float* out_val, int64_t ldo, void* stream) {
    return topk_launch(x, rows, cols, ldx, row_div, k, out_idx, out_val, ldo, (hipStream_t)stream);
}

REIDMI_API int64_t reidmi_search_workspace_bytes(int64_t Q, int64_t G, int64_t D, int k) {
    SrPlan p;
    return D > 0 && sr_plan(Q, G, k, 0, 0, &p) ? sr_ws_bytes(Q, G, p) : -1;
}

REIDMI_API int reidmi_search_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                 int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams,
                                 const int64_t* g_pids, const int64_t* g_cams, int32_t* out_idx, float* out_dist,
                                 int64_t ldo, void* ws, int64_t ws_bytes, void* stream) {
    return search_impl(q, Q, ldq, g, G, ldg, D, k, q_pids, q_cams, g_pids, g_cams, nullptr, nullptr, nullptr, 1, 0,
                       out_idx, out_dist, ldo, ws, ws_bytes, 0, 0, nullptr, stream);
}

REIDMI_API int reidmi_search_bounded_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G,
                                         int64_t ldg, int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams,
                                         const int64_t* g_pids, const int64_t* g_cams, const float* bound_dist,
                                         const int32_t* bound_idx, int64_t ldb, int64_t index_base, int32_t* out_idx,
                                         float* out_dist, int64_t ldo, void* ws, int64_t ws_bytes, void* stream) {
    return search_impl(q, Q, ldq, g, G, ldg, D, k, q_pids, q_cams, g_pids, g_cams, nullptr, bound_dist, bound_idx,
                       ldb, index_base, out_idx, out_dist, ldo, ws, ws_bytes, 0, 0, nullptr, stream);
}

REIDMI_API int reidmi_search_filtered_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G,
                                          int64_t ldg, int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams,
                                          const int64_t* g_pids, const int64_t* g_cams,
                                          const reidmi_search_filter* flt, const float* bound_dist,
                                          const int32_t* bound_idx, int64_t ldb, int64_t index_base, int32_t* out_idx,
                                          float* out_dist, int64_t ldo, void* ws, int64_t ws_bytes, void* stream) {
    return search_impl(q, Q, ldq, g, G, ldg, D, k, q_pids, q_cams, g_pids, g_cams, flt, bound_dist, bound_idx, ldb,
                       index_base, out_idx, out_dist, ldo, ws, ws_bytes, 0, 0, nullptr, stream);
}

REIDMI_API int reidmi_search_merge_f32(const int32_t* in_idx, const float* in_dist, int S, int64_t Q, int k_in,
                                       int64_t list_stride, int64_t ldi, const int64_t* base, int k,
                                       int32_t* out_idx, float* out_dist, int64_t ldo, void* stream) {
    return search_merge_launch(in_idx, in_dist, S, Q, k_in, list_stride, ldi, base, k, out_idx, out_dist, ldo, stream);
}

#ifdef REIDMI_TOOLS
// reidmi_search_f32 with a forced number of gallery ranges and list capacity (0 = the launcher's
// choice) and the kernel's counters (tests; tools library, include/reidmi_tools.h).
REIDMI_API int64_t reidmi_search_ex_workspace_bytes(int64_t Q, int64_t G, int64_t D, int k, int splits, int cap) {
    SrPlan p;
    return D > 0 && sr_plan(Q, G, k, splits, cap, &p) ? sr_ws_bytes(Q, G, p) : -1;
}

REIDMI_API int reidmi_search_f32_ex(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                    int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams,
                                    const int64_t* g_pids, const int64_t* g_cams, int32_t* out_idx, float* out_dist,
                                    int64_t ldo, void* ws, int64_t ws_bytes, int splits, int cap, int32_t* stats,
                                    void* stream) {
    return search_impl(q, Q, ldq, g, G, ldg, D, k, q_pids, q_cams, g_pids, g_cams, nullptr, nullptr, nullptr, 1, 0,
                       out_idx, out_dist, ldo, ws, ws_bytes, splits, cap, stats, stream);
}

REIDMI_API int reidmi_search_bounded_f32_ex(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G,
                                            int64_t ldg, int64_t D, int k, const int64_t* q_pids,
                                            const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                                            const float* bound_dist, const int32_t* bound_idx, int64_t ldb,
                                            int64_t index_base, int32_t* out_idx, float* out_dist, int64_t ldo,
                                            void* ws, int64_t ws_bytes, int splits, int cap, int32_t* stats,
                                            void* stream) {
    return search_impl(q, Q, ldq, g, G, ldg, D, k, q_pids, q_cams, g_pids, g_cams, nullptr, bound_dist, bound_idx,
                       ldb, index_base, out_idx, out_dist, ldo, ws, ws_bytes, splits, cap, stats, stream);
}

// reidmi_search_filtered_f32 with the same forced splits, capacity and counters.
REIDMI_API int reidmi_search_filtered_f32_ex(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G,
                                             int64_t ldg, int64_t D, int k, const int64_t* q_pids,
                                             const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                                             const reidmi_search_filter* flt, const float* bound_dist,
                                             const int32_t* bound_idx, int64_t ldb, int64_t index_base,
                                             int32_t* out_idx, float* out_dist, int64_t ldo, void* ws,
                                             int64_t ws_bytes, int splits, int cap, int32_t* stats, void* stream) {
    return search_impl(q, Q, ldq, g, G, ldg, D, k, q_pids, q_cams, g_pids, g_cams, flt, bound_dist, bound_idx, ldb,
                       index_base, out_idx, out_dist, ldo, ws, ws_bytes, splits, cap, stats, stream);
}
#endif
