// evalfeat.hip — per-query CMC / AP of the CLIP-ReID eval path from the features, without the
// Q x G matrix (reidmi_eval_feat_f32 and its stages reidmi_evf_*; include/reidmi.h).
//
// eval_rows_wg_kernel (eval.hip) sorts a query's matches by (distance, index), bins every kept
// gallery item by how many matches precede it and scans that histogram into kept-ranks.  The
// histogram is a sum of integer counts over gallery columns, so the binning can run in the
// epilogue of the distance tile, block by block and GPU by GPU:
//   matches   label compares, then each match's distance by the scalar chain the tile is bit-equal to
//   sort      each query's list by select.h's key order
//   count     the distance tile of search_f32_kernel; epilogue: hist[i][#matches before (v, j)]++
//   finish    scan + eval.hip's AP summers (evf_finish_launch, defined there)
// The distance tile is distance.h's (the distance kernels' bits), the key order select.h's.
#include "backend.h"
#include "distance.h"
#include "select.h"

namespace reidmi {

// ------------------------------------------------------------------------ matches
// One workgroup per 128-query band and chunk of EVF_MCH gallery items: the band's labels sit in
// LDS, every thread holds EVF_MU gallery labels and compares them with the 128 queries (LDS
// broadcast reads).  A hit is rare (a query's matches are a handful among the gallery), so the
// atomics on the per-query counts do not contend.  The entry's distance is filled afterwards.
constexpr int EVF_MU = 8, EVF_MCH = 256 * EVF_MU;

__global__ __launch_bounds__(256) void evf_matches_kernel(DmLabels lab, int64_t Q, int64_t Gb, int64_t bands,
                                                          int64_t base, int cap, float2* __restrict__ pos,
                                                          int32_t* __restrict__ pos_cnt,
                                                          int32_t* __restrict__ junk_cnt,
                                                          int32_t* __restrict__ overflow) {
    __shared__ int64_t s_qp[DM_BM], s_qc[DM_BM];
    const int tid = threadIdx.x;
    const int64_t band = blockIdx.x % bands, chunk = blockIdx.x / bands, bm = band * DM_BM;
    const int nq = Q - bm < DM_BM ? (int)(Q - bm) : DM_BM;
    if (tid < nq) {
        s_qp[tid] = lab.qp[bm + tid];
        s_qc[tid] = lab.qc[bm + tid];
    }
    int64_t gp[EVF_MU];
    bool in[EVF_MU];
#pragma unroll
    for (int u = 0; u < EVF_MU; u++) {
        const int64_t j = chunk * EVF_MCH + u * 256 + tid;
        in[u] = j < Gb;
        gp[u] = lab.gp[in[u] ? j : Gb - 1];
    }
    __syncthreads();
    for (int i = 0; i < nq; i++) {
        const int64_t qp = s_qp[i];
#pragma unroll
        for (int u = 0; u < EVF_MU; u++) {
            if (!(in[u] && gp[u] == qp)) continue;
            const int64_t j = chunk * EVF_MCH + u * 256 + tid;
            if (lab.gc[j] == s_qc[i]) {  // removed (evaluate.py:46-48)
                atomicAdd(&junk_cnt[bm + i], 1);
            } else {
                const int p = atomicAdd(&pos_cnt[bm + i], 1);
                if (p < cap) pos[(bm + i) * cap + p] = make_float2(0.0f, __int_as_float((int)(base + j)));
                else *overflow = 1;
            }
        }
    }
}

// The distance of entry (i, j) by the chain the distance tile is bit-equal to: fmaf over k
// ascending from +0, then dm_value.  VEC: rows 16-byte aligned, D % 4 == 0 (dm2_ok).
template <bool VEC>
__device__ __forceinline__ float evf_dist(const float* __restrict__ a, const float* __restrict__ b, int64_t D,
                                          float qq, float gg) {
    float acc = 0.0f;
    int64_t k = 0;
    if constexpr (VEC) {
        // unrolled so that many row loads are in flight ahead of the (sequential) fma chain
#pragma unroll 8
        for (; k + 4 <= D; k += 4) {
            const float4 x = *(const float4*)(a + k), y = *(const float4*)(b + k);
            acc = __builtin_fmaf(x.x, y.x, acc);
            acc = __builtin_fmaf(x.y, y.y, acc);
            acc = __builtin_fmaf(x.z, y.z, acc);
            acc = __builtin_fmaf(x.w, y.w, acc);
        }
    }
    for (; k < D; k++) acc = __builtin_fmaf(a[k], b[k], acc);
    return dm_value(acc, qq, gg);
}

// One thread per list entry; the entries of this block are those with an index in [base, base + Gb).
template <bool VEC>
__global__ __launch_bounds__(256) void evf_fill_kernel(const float* __restrict__ q, const float* __restrict__ g,
                                                       const float* __restrict__ qq, const float* __restrict__ gg,
                                                       int64_t Q, int64_t Gb, int64_t D, int64_t ldq, int64_t ldg,
                                                       int64_t base, int cap, float2* __restrict__ pos,
                                                       const int32_t* __restrict__ pos_cnt) {
    const int64_t total = Q * cap;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / cap;
        const int t = (int)(e - i * cap);
        if (t >= pos_cnt[i]) continue;
        const int64_t j = (int64_t)kv_idx(pos[e]) - base;
        if (j < 0 || j >= Gb) continue;
        pos[e].x = evf_dist<VEC>(q + i * ldq, g + j * ldg, D, qq[i], gg[j]);
    }
}

// ------------------------------------------------------------------------- append
__global__ __launch_bounds__(256) void evf_append_kernel(float2* __restrict__ dst, int32_t* __restrict__ dst_cnt,
                                                         const float2* __restrict__ src,
                                                         const int32_t* __restrict__ src_cnt, int cap,
                                                         int32_t* __restrict__ overflow) {
    const int64_t i = blockIdx.x;
    const int nd = dst_cnt[i], ns = src_cnt[i];
    const int have = nd < cap ? nd : cap, take = ns < cap ? ns : cap;  // entries held on either side
    for (int t = threadIdx.x; t < take; t += 256)
        if (have + t < cap) dst[i * cap + have + t] = src[i * cap + t];
    __syncthreads();  // every thread has read the count
    if (threadIdx.x == 0) {
        dst_cnt[i] = nd + ns;
        if ((int64_t)nd + ns > cap) *overflow = 1;
    }
}

// --------------------------------------------------------------------------- sort
// One workgroup per query.  Lists of up to EVF_SORT_LDS entries: select.h's bitonic sort in LDS.
// Longer ones: the same network in its all-ascending form, in place in global memory — the first
// step of every merge pairs t with its mirror in the block (t ^ (k - 1)), the rest pair t with
// t ^ j, every exchange puts the smaller key first, and a partner past the list's end counts as
// +inf and is left alone, so no power-of-two padding (and no scratch) is needed.
constexpr int EVF_SORT_LDS = 512;

__global__ __launch_bounds__(256) void evf_sort_kernel(float2* pos, const int32_t* __restrict__ pos_cnt, int cap) {
    __shared__ float sv[EVF_SORT_LDS];
    __shared__ int si[EVF_SORT_LDS];
    const int64_t i = blockIdx.x;
    const int c = pos_cnt[i], n = c < cap ? c : cap;
    float2* row = pos + i * cap;
    if (n < 2) return;
    if (n <= EVF_SORT_LDS) {
        const int P = pow2_ceil(n);
        for (int t = threadIdx.x; t < P; t += 256) {
            const float2 e = t < n ? row[t] : make_float2(__builtin_inff(), __int_as_float(0x7fffffff));
            sv[t] = e.x;
            si[t] = kv_idx(e);
        }
        __syncthreads();
        bitonic_sort_kv(sv, si, P);
        for (int t = threadIdx.x; t < n; t += 256) row[t] = make_float2(sv[t], __int_as_float(si[t]));
        return;
    }
    for (int64_t k = 2; (k >> 1) < n; k <<= 1) {
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            const int64_t mask = j == (k >> 1) ? k - 1 : j;
            for (int64_t t = threadIdx.x; t < n; t += 256) {
                const int64_t o = t ^ mask;
                if (o > t && o < n) {
                    const float2 a = row[t], b = row[o];
                    if (key_less(b.x, kv_idx(b), a.x, kv_idx(a))) { row[t] = b; row[o] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// -------------------------------------------------------------------------- count
// distance.h's band-and-range walk: a workgroup owns one 128-row query band and one contiguous
// gallery range [c0, c1) of the block and walks it in 128-column tiles with the distance kernels'
// mainloops, so v below has the distance kernel's bits.  Row state in LDS: the squared norm, the
// labels, the number of matches and the LAST match's key.  Epilogue per element: removed items
// and everything after the row's last match end at one compare (most elements, when the features
// are any good: what lies before a query's last match is a small part of the gallery); the rest
// find b = #matches with a smaller key by binary search over the row's sorted list (L2-resident:
// Q * cap * 8 bytes) and add 1 to hist[i][b] (an L2 atomic; integer, so any order gives the same
// sum).  LDS: 33 024 B of operand stages + 2.5 KB of row state + 2 KB of labels: four workgroups
// per CU, as the search.
template <bool PIPE>
__global__ __launch_bounds__(256, DM2_MINWG) void evf_count_kernel(
    const float* __restrict__ q, const float* __restrict__ g, const float* __restrict__ qq,
    const float* __restrict__ gg, int64_t Q, int64_t Gb, int64_t D, int64_t ldq, int64_t ldg, DmLabels lab,
    int64_t range_len, int64_t base, int cap, const float2* __restrict__ pos, const int32_t* __restrict__ pos_cnt,
    int32_t* __restrict__ hist) {
    __shared__ float smem[DM_SMEM];
    __shared__ float s_qq[DM_BM], s_lv[DM_BM];
    __shared__ int s_li[DM_BM], s_m[DM_BM];
    __shared__ int64_t s_qp[DM_BM], s_qc[DM_BM];
    const DmThread t = dm_thread();
    const int tid = t.tid, lane = t.lane, wm = t.wm, wn = t.wn;
    const DmWalk w = dm_walk(Q, Gb, range_len);
    const int64_t bm = w.bm, c0 = w.c0, c1 = w.c1;
    if (tid < DM_BM) {
        const bool in = bm + tid < Q;
        int m = in ? pos_cnt[bm + tid] : 0;
        m = m < cap ? m : cap;
        // no match: nothing lies before the last one
        const float2 e = m > 0 ? pos[(bm + tid) * cap + m - 1] : make_float2(-__builtin_inff(), __int_as_float(-1));
        s_m[tid] = m;
        s_lv[tid] = e.x;
        s_li[tid] = kv_idx(e);
        s_qq[tid] = in ? qq[bm + tid] : 0.0f;
        s_qp[tid] = in ? lab.qp[bm + tid] : 0;
        s_qc[tid] = in ? lab.qc[bm + tid] : 0;
    }
    __syncthreads();
    for (int64_t bn = c0; bn < c1; bn += DM_BN) {
        f32x16 acc[2][2];
        dm_acc_zero(acc);
        dm_tile<PIPE>(t, q, g, Q, c1, D, ldq, ldg, bm, bn, smem, acc);
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            const int64_t j = bn + dm_lane_col(wn, nt, lane);
            if (j >= c1) continue;
            const int jg = (int)(base + j);
            const float ggj = gg[j];
            int64_t gpj = 0, gcj = 0;
            bool lab_loaded = false;
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int il = dm_lane_row(wm, mt, r, lane);
                    if (bm + il >= Q) continue;
                    const float v = dm_value(acc[mt][nt][r], s_qq[il], ggj);
                    const float lv = s_lv[il];
                    if (!(v <= lv)) continue;                  // after the last match
                    if (v == lv && jg > s_li[il]) continue;    // tied with it, after it
                    if (!lab_loaded) { gpj = lab.gp[j]; gcj = lab.gc[j]; lab_loaded = true; }
                    if (gpj == s_qp[il] && gcj == s_qc[il]) continue;  // evaluate.py:46-48
                    const float2* row = pos + (bm + il) * cap;
                    int lo = 0, hi = s_m[il];
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        const float2 e = row[mid];
                        if (key_less(e.x, kv_idx(e), v, jg)) lo = mid + 1; else hi = mid;
                    }
                    atomicAdd(&hist[(bm + il) * ((int64_t)cap + 1) + lo], 1);
                }
        }
    }
}

// ------------------------------------------------------------------------- launchers
// The argument checks every entry point shares; all before any HIP call.
static int evf_check(const char* who, int64_t Q, int64_t Gb, int64_t D, int64_t ldq, int64_t ldg, int64_t base,
                     int cap, const DmLabels& lab) {
    const std::string w(who);
    RM_REQUIRE(Q >= 0 && Q < (1ll << 31) && Gb > 0 && D > 0, w + ": bad shape (need Q >= 0, G > 0, D > 0)");
    RM_REQUIRE(ldq >= D && ldg >= D, w + ": row pitches must be >= D");
    RM_REQUIRE(cap >= 1, w + ": need cap >= 1");
    RM_REQUIRE(base >= 0 && base + Gb < (1ll << 31) && Gb < (1ll << 31),
               w + ": gallery indices must fit int32 (base >= 0, base + G < 2^31)");
    RM_REQUIRE(lab.qp && lab.qc && lab.gp && lab.gc, w + ": all four label arrays are required");
    return OK;
}

static int evf_matches_run(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t Gb, int64_t ldg,
                           int64_t D, const DmLabels& lab, const float* qq, const float* gg, int64_t base, int cap,
                           float2* pos, int32_t* pos_cnt, int32_t* junk_cnt, int32_t* overflow, hipStream_t s) {
    const int64_t bands = (Q + DM_BM - 1) / DM_BM, chunks = (Gb + EVF_MCH - 1) / EVF_MCH;
    RM_REQUIRE(bands * chunks < (1ll << 31), "evf_matches: too many (query band, gallery chunk) pairs for one launch");
    hipLaunchKernelGGL(evf_matches_kernel, dim3((unsigned)(bands * chunks)), dim3(256), 0, s, lab, Q, Gb, bands, base,
                       cap, pos, pos_cnt, junk_cnt, overflow);
    RM_LAUNCHED();
    const int64_t blocks = (Q * cap + 255) / 256;
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
    RM_BOOL_SWITCH(dm2_ok(q, ldq, g, ldg, D), VEC,
                   hipLaunchKernelGGL(evf_fill_kernel<VEC>, grid, dim3(256), 0, s, q, g, qq, gg, Q, Gb, D, ldq, ldg,
                                      base, cap, pos, (const int32_t*)pos_cnt));
    RM_LAUNCHED();
    return OK;
}

static int evf_sort_run(float2* pos, const int32_t* pos_cnt, int64_t Q, int cap, hipStream_t s) {
    hipLaunchKernelGGL(evf_sort_kernel, dim3((unsigned)Q), dim3(256), 0, s, pos, pos_cnt, cap);
    RM_LAUNCHED();
    return OK;
}

// The gallery ranges of the count: distance.h's dm_walk_plan.
static int evf_count_run(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t Gb, int64_t ldg, int64_t D,
                         const DmLabels& lab, const float* qq, const float* gg, int64_t base, int cap,
                         const float2* pos, const int32_t* pos_cnt, int32_t* hist, hipStream_t s) {
    const int64_t bands = (Q + DM_BM - 1) / DM_BM, tiles = (Gb + DM_BN - 1) / DM_BN;
    int64_t S, range_len;
    dm_walk_plan(bands, tiles, &S, &range_len);
    RM_REQUIRE(bands * S < (1ll << 31), "evf_count: too many query bands for one launch");
    const dim3 grid((unsigned)(bands * S));
    RM_BOOL_SWITCH(dm2_ok(q, ldq, g, ldg, D), PIPE,
                   hipLaunchKernelGGL(evf_count_kernel<PIPE>, grid, dim3(256), 0, s, q, g, qq, gg, Q, Gb, D, ldq, ldg,
                                      lab, range_len, base, cap, pos, pos_cnt, hist));
    RM_LAUNCHED();
    return OK;
}

// one-call workspace: norms | pos | pos_cnt, junk_cnt, hist (zeroed together)
struct EvfWs {
    int64_t pos_off, zero_off, zero_bytes, bytes;
};
static bool evf_ws(int64_t Q, int64_t G, int64_t D, int cap, EvfWs* w) {
    if (Q < 0 || Q >= (1ll << 31) || G <= 0 || G >= (1ll << 31) || D <= 0 || cap < 1) return false;
    w->pos_off = dm_norm_bytes(Q, G);
    w->zero_off = w->pos_off + Q * cap * 8;
    w->zero_bytes = (Q * 8 + Q * ((int64_t)cap + 1) * 4 + 15) / 16 * 16;
    w->bytes = w->zero_off + w->zero_bytes;
    return true;
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int64_t reidmi_evf_workspace_bytes(int64_t Q, int64_t Gb) {
    return Q >= 0 && Gb > 0 ? dm_norm_bytes(Q, Gb) : -1;
}

REIDMI_API int reidmi_evf_matches(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t Gb, int64_t ldg,
                                  int64_t D, const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                                  const int64_t* g_cams, int64_t base, int cap, void* pos, int32_t* pos_cnt,
                                  int32_t* junk_cnt, int32_t* overflow, void* ws, int64_t ws_bytes, void* stream) {
    const DmLabels lab{q_pids, q_cams, g_pids, g_cams};
    RM_TRY(evf_check("evf_matches", Q, Gb, D, ldq, ldg, base, cap, lab));
    RM_REQUIRE(ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= dm_norm_bytes(Q, Gb),
               "evf_matches: workspace (reidmi_evf_workspace_bytes, 16-byte aligned) required");
    RM_REQUIRE(pos != nullptr && ((uintptr_t)pos & 7) == 0 && pos_cnt != nullptr && junk_cnt != nullptr &&
                   overflow != nullptr,
               "evf_matches: pos (8-byte aligned), pos_cnt, junk_cnt and overflow required");
    RM_REQUIRE(q != nullptr && g != nullptr, "evf_matches: features required");
    if (Q == 0) return OK;
    hipStream_t s = (hipStream_t)stream;
    float* qq = (float*)ws;
    float* gg = qq + Q;
    RM_TRY(dm_norms(q, Q, ldq, g, Gb, ldg, D, qq, gg, s));
    return evf_matches_run(q, Q, ldq, g, Gb, ldg, D, lab, qq, gg, base, cap, (float2*)pos, pos_cnt, junk_cnt, overflow,
                           s);
}

REIDMI_API int reidmi_evf_append(void* dst_pos, int32_t* dst_cnt, const void* src_pos, const int32_t* src_cnt,
                                 int64_t Q, int cap, int32_t* overflow, void* stream) {
    RM_REQUIRE(Q >= 0 && Q < (1ll << 31), "evf_append: bad Q");
    RM_REQUIRE(cap >= 1, "evf_append: need cap >= 1");
    RM_REQUIRE(dst_pos != nullptr && dst_cnt != nullptr && src_pos != nullptr && src_cnt != nullptr &&
                   overflow != nullptr && (((uintptr_t)dst_pos | (uintptr_t)src_pos) & 7) == 0,
               "evf_append: dst_pos, dst_cnt, src_pos, src_cnt (lists 8-byte aligned) and overflow required");
    if (Q == 0) return OK;
    hipLaunchKernelGGL(evf_append_kernel, dim3((unsigned)Q), dim3(256), 0, (hipStream_t)stream, (float2*)dst_pos,
                       dst_cnt, (const float2*)src_pos, src_cnt, cap, overflow);
    RM_LAUNCHED();
    return OK;
}

REIDMI_API int reidmi_evf_sort(void* pos, const int32_t* pos_cnt, int64_t Q, int cap, void* stream) {
    RM_REQUIRE(Q >= 0 && Q < (1ll << 31), "evf_sort: bad Q");
    RM_REQUIRE(cap >= 1, "evf_sort: need cap >= 1");
    RM_REQUIRE(pos != nullptr && ((uintptr_t)pos & 7) == 0 && pos_cnt != nullptr,
               "evf_sort: pos (8-byte aligned) and pos_cnt required");
    if (Q == 0) return OK;
    return evf_sort_run((float2*)pos, pos_cnt, Q, cap, (hipStream_t)stream);
}

REIDMI_API int reidmi_evf_count(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t Gb, int64_t ldg,
                                int64_t D, const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                                const int64_t* g_cams, int64_t base, int cap, const void* pos, const int32_t* pos_cnt,
                                int32_t* hist, void* ws, int64_t ws_bytes, void* stream) {
    const DmLabels lab{q_pids, q_cams, g_pids, g_cams};
    RM_TRY(evf_check("evf_count", Q, Gb, D, ldq, ldg, base, cap, lab));
    RM_REQUIRE(ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= dm_norm_bytes(Q, Gb),
               "evf_count: workspace (reidmi_evf_workspace_bytes, 16-byte aligned) required");
    RM_REQUIRE(pos != nullptr && ((uintptr_t)pos & 7) == 0 && pos_cnt != nullptr && hist != nullptr,
               "evf_count: pos (8-byte aligned), pos_cnt and hist required");
    RM_REQUIRE(q != nullptr && g != nullptr, "evf_count: features required");
    if (Q == 0) return OK;
    hipStream_t s = (hipStream_t)stream;
    float* qq = (float*)ws;
    float* gg = qq + Q;
    RM_TRY(dm_norms(q, Q, ldq, g, Gb, ldg, D, qq, gg, s));
    return evf_count_run(q, Q, ldq, g, Gb, ldg, D, lab, qq, gg, base, cap, (const float2*)pos, pos_cnt, hist, s);
}

REIDMI_API int reidmi_evf_finish(const int32_t* pos_cnt, int32_t* hist, const int32_t* junk_cnt, int64_t Q, int cap,
                                 int64_t G_total, int32_t* overflow, int32_t* valid, int64_t* first, int64_t* last,
                                 int32_t* npos, double* ap, int64_t* nkept, void* stream) {
    return evf_finish_launch(pos_cnt, hist, junk_cnt, Q, cap, G_total, overflow, valid, first, last, npos, ap, nkept,
                             (hipStream_t)stream);
}

REIDMI_API int64_t reidmi_eval_feat_workspace_bytes(int64_t Q, int64_t G, int64_t D, int cap) {
    EvfWs w;
    return evf_ws(Q, G, D, cap, &w) ? w.bytes : -1;
}

REIDMI_API int reidmi_eval_feat_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                    int64_t D, const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                                    const int64_t* g_cams, int cap, int32_t* valid, int64_t* first, int64_t* last,
                                    int32_t* npos, double* ap, int64_t* nkept, int32_t* overflow, void* ws,
                                    int64_t ws_bytes, void* stream) {
    const DmLabels lab{q_pids, q_cams, g_pids, g_cams};
    RM_TRY(evf_check("eval_feat", Q, G, D, ldq, ldg, 0, cap, lab));
    EvfWs w;
    RM_REQUIRE(evf_ws(Q, G, D, cap, &w) && ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= w.bytes,
               "eval_feat: workspace (reidmi_eval_feat_workspace_bytes, 16-byte aligned) required");
    RM_REQUIRE(valid != nullptr && first != nullptr && ap != nullptr && nkept != nullptr && overflow != nullptr,
               "eval_feat: valid, first, ap, nkept and overflow required");
    RM_REQUIRE(q != nullptr && g != nullptr, "eval_feat: features required");
    if (Q == 0) return OK;
    hipStream_t s = (hipStream_t)stream;
    float* qq = (float*)ws;
    float* gg = qq + Q;
    float2* pos = (float2*)((char*)ws + w.pos_off);
    int32_t* pos_cnt = (int32_t*)((char*)ws + w.zero_off);
    int32_t* junk_cnt = pos_cnt + Q;
    int32_t* hist = junk_cnt + Q;
    RM_CHECK_HIP(hipMemsetAsync(pos_cnt, 0, (size_t)w.zero_bytes, s));
    RM_CHECK_HIP(hipMemsetAsync(overflow, 0, sizeof(int32_t), s));
    RM_TRY(dm_norms(q, Q, ldq, g, G, ldg, D, qq, gg, s));
    RM_TRY(evf_matches_run(q, Q, ldq, g, G, ldg, D, lab, qq, gg, 0, cap, pos, pos_cnt, junk_cnt, overflow, s));
    RM_TRY(evf_sort_run(pos, pos_cnt, Q, cap, s));
    RM_TRY(evf_count_run(q, Q, ldq, g, G, ldg, D, lab, qq, gg, 0, cap, pos, pos_cnt, hist, s));
    return evf_finish_launch(pos_cnt, hist, junk_cnt, Q, cap, G, overflow, valid, first, last, npos, ap, nkept, s);
}
