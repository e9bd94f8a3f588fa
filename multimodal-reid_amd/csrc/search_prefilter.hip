// search_prefilter.hip — reidmi_search_bounded_f32's rank lists from an fp16 pre-filter, on gfx950:
// the fp16 MFMA product bounds every exact distance (the error model above rank_select1_kernel,
// prefilter.hip), only the pairs that can still be among a row's k nearest survive the GEMM's
// epilogue (EPI_RRSV, gemm_rrsv.h), and the survivors are recomputed with the exact chain.
//
// Per pass of query rows:
//   (a) hi of the rows against every S-th gallery item           gemm_f16(EPI_RRHI)
//   (b) the row's threshold T and its survivor record            sp_threshold_kernel
//   (c) the survivors {j : hi_ij - w_i <= T} of every row        gemm_f16(EPI_RRSV), rectangular tile list
//   (d) the exact distances of the candidates, the k smallest    sp_select_kernel
//
// Why the lists are the exact search's.  The exact distance d_ij (the distance kernel's bits) lies
// in [fl(hi_ij - w_i), hi_ij] (rr_width).  "Admitted" is admit.h's sr_admit: the label rule and
// the filter's clauses, one definition for this file and the exact search.  (b): U = the k-th
// smallest hi among the admitted sample items; those k items have d <= U, so each of the k nearest
// admissible items (admitted, and under the bound) has d <= U, and d <= the bound's distance because
// it is admissible: d <= T = min(U, bound), hence fl(hi - w) <= T and the pair survives (c), which
// knows no clause: it keeps admitted and non-admitted pairs alike.  (d) repeats the argument on the
// survivors (the k-th smallest hi of the admitted ones, capped by T), computes the exact distance of
// what is left, applies reidmi_search_bounded_f32's bound on the exact key and selects by the unique
// key (d, j): the order in which the epilogue's atomics appended the survivors cannot show.
// A selective filter leaves few admitted sample items, so U is loose (fewer than k of them: +inf)
// and the survivor lists, which hold non-admitted pairs too, overflow: such rows go to the exact
// filtered search.  Correct, and slower than calling the exact search at once.
// A row whose list overflows (more than RR_SV_CAP survivors), or that holds a non-finite bound, is
// marked in need[] and left to the exact search; so is every row when a feature is outside fp16's range.
#include "admit.h"
#include "backend.h"
#include "prefilter.h"
#include "select.h"

namespace reidmi {

constexpr int SP_K_MAX = 128;               // reidmi_search_f32's
constexpr int64_t SP_PASS_BYTES = 1ll << 30;  // per-pass state (sample bounds + survivor lists) aimed at

struct SpBound {  // reidmi_search_bounded_f32's (search.hip SrBound)
    const float* dist;
    const int32_t* idx;
    int64_t ld, base;
};
// device state of one call (workspace): the range flag and the statistics' accumulators
struct SpState {
    float nmax2[2];  // the gallery's largest norm and squared norm
    int32_t range_ok, need_rows, max_survivors, pad;
    unsigned long long rescored;
};

__global__ void sp_init_kernel(SpState* st) {
    st->range_ok = 1;
    st->need_rows = 0;
    st->max_survivors = 0;
    st->pad = 0;
    st->rescored = 0;
}

__global__ void sp_sqrt_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) y[t] = sqrtf(x[t]);
}

// (b) One workgroup per row r of the pass (query row0 + r): U = the K-th smallest hi among the
// sample items (position t = gallery item t S) that are admitted (sr_admit), T = min(U, the row's
// bound distance) (a NaN or -inf bound: -inf, nothing survives), and the survivor epilogue's
// row record (s, n, hi_max(T), +inf): with lb = +inf the epilogue's test keeps exactly hi <= hi_max.
// Fewer than K such sample items and no finite bound: T = +inf, everything survives (the row
// overflows unless the gallery fits a list).  A non-finite sample bound marks the row (cnt past cap).
__global__ __launch_bounds__(256) void sp_threshold_kernel(const float* __restrict__ hs, int64_t ns, int S,
                                                           const float* __restrict__ qq,
                                                           const float* __restrict__ qn,
                                                           const SpState* __restrict__ st, int64_t row0, int K,
                                                           float c_rel, float c_abs, float c_d, SrFilter flt,
                                                           SpBound bnd, float4* __restrict__ meta,
                                                           float* __restrict__ wrow, float* __restrict__ trow,
                                                           int32_t* __restrict__ cnt, int cap) {
    __shared__ TkLds L;
    const int64_t r = blockIdx.x, i = row0 + r;
    const float* row = hs + r * ns;
    int bad = 0;
    for (int64_t t = threadIdx.x; t < ns; t += blockDim.x) bad |= !(fabsf(row[t]) < __builtin_inff());
    bad = __syncthreads_or(bad);
    const bool labels = flt.qp != nullptr, clauses = sr_has_clauses(flt);
    if (labels || clauses) {
        const SrRow qside = sr_row(flt, labels, clauses, i);
        topk_row_dev([&](int64_t t) { return row[t]; }, ns, K, L, [&](float, int t) {
            return sr_admit(flt, labels, clauses, qside, sr_item(flt, labels, clauses, (int64_t)t * S));
        });
    } else {
        topk_row_dev([&](int64_t t) { return row[t]; }, ns, K, L);
    }
    if (threadIdx.x == 0) {
        const float s = qq[i], n = qn[i];
        const float w = rr_width(s, n, st->nmax2[0], st->nmax2[1], c_rel, c_abs, c_d);
        float T = L.s_nsel == K ? L.sv[K - 1] : __builtin_inff();
        if (bnd.dist != nullptr) {
            const float bd = bnd.dist[i * bnd.ld];
            T = bd == bd ? fminf(T, bd) : -__builtin_inff();
        }
        const float hmax = fabsf(T) < __builtin_inff() ? rr_hmax(T, w) : T;
        meta[r] = make_float4(s, n, hmax, __builtin_inff());
        wrow[r] = w;
        trow[r] = T;
        cnt[r] = bad ? cap + 1 : 0;
    }
}

// (d) One workgroup per row: the row's survivor list (cnt, list: (gallery item, hi bits), any
// order) -> out_idx / out_dist [K], or need = 1.  Two sorts in LDS by the unique key (value, item):
// the survivors by hi, then the candidates by their exact distance.  LDS: RR_SV_CAP x 8 B = 32 KiB
// (four workgroups, 16 waves, per CU beside nothing else; the chain is latency-bound, so the
// waves matter more than the bytes).
__global__ __launch_bounds__(256) void sp_select_kernel(const int32_t* __restrict__ cnt,
                                                        const int2* __restrict__ list, int cap,
                                                        const float* __restrict__ wrow,
                                                        const float* __restrict__ trow,
                                                        const float* __restrict__ q, int64_t ldq,
                                                        const float* __restrict__ g, int64_t ldg, int D, bool vec,
                                                        const float* __restrict__ qq,
                                                        const float* __restrict__ gg, int64_t row0, int64_t G,
                                                        int K, SrFilter flt, SpBound bnd, SpState* __restrict__ st,
                                                        int32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                        int64_t ldo, int32_t* __restrict__ need) {
    __shared__ float sv[RR_SV_CAP];
    __shared__ int si[RR_SV_CAP];
    __shared__ int s_rm, s_nc;
    const int64_t r = blockIdx.x, i = row0 + r;
    const int n = cnt[r];
    if (threadIdx.x == 0) atomicMax(&st->max_survivors, n);  // (cap + 1: marked by the sample)
    if (n > cap || st->range_ok == 0) {  // overflow, a non-finite sample bound, or features beyond fp16
        if (threadIdx.x == 0) {
            need[i] = 1;
            atomicAdd(&st->need_rows, 1);
        }
        return;
    }
    const int2* lr = list + r * (int64_t)cap;
    const bool labels = flt.qp != nullptr, clauses = sr_has_clauses(flt);
    const SrRow qside = sr_row(flt, labels, clauses, i);
    const int P = pow2_ceil(n < 2 ? 2 : n);
    if (threadIdx.x == 0) { s_rm = 0; s_nc = 0; }
    __syncthreads();
    int bad = 0, removed = 0;
    for (int t = threadIdx.x; t < P; t += blockDim.x) {
        float h = __builtin_inff();
        int j = 0x7fffffff;
        if (t < n) {
            const int2 e = lr[t];
            h = __builtin_bit_cast(float, e.y);
            j = e.x;
            bad |= !(fabsf(h) < __builtin_inff());
            if ((labels || clauses) &&
                !sr_admit(flt, labels, clauses, qside, sr_item(flt, labels, clauses, j))) {  // never a candidate
                h = __builtin_inff();
                j = 0x7fffffff;
                removed++;
            }
        }
        sv[t] = h;
        si[t] = j;
    }
    if (removed) atomicAdd(&s_rm, removed);
    if (__syncthreads_or(bad)) {  // a non-finite bound: the exact search
        if (threadIdx.x == 0) {
            need[i] = 1;
            atomicAdd(&st->need_rows, 1);
        }
        return;
    }
    bitonic_sort_kv(sv, si, P);  // ascending (hi, item); the removed ones last
    const int m = n - s_rm;
    const float w = wrow[r], T = trow[r];
    const float tau = m >= K ? fminf(sv[K - 1], T) : T;
    // the candidates: the prefix with lo = fl(hi - w) <= tau
    int pc = 0;
    for (int t = threadIdx.x; t < m; t += blockDim.x)
        if (sv[t] - w <= tau) pc = t + 1;
    if (pc) atomicMax(&s_nc, pc);
    __syncthreads();
    const int nc = s_nc;
    // the row's bound as the exact search's kernel holds it (search.hip): the threshold key (tv, ti),
    // the index moved to this gallery's local j
    float tv = __builtin_inff();
    int ti = 0x7fffffff;
    if (bnd.dist != nullptr) {
        tv = bnd.dist[i * bnd.ld];
        if (bnd.idx != nullptr) {
            const int64_t l = (int64_t)bnd.idx[i * bnd.ld] - bnd.base;
            ti = l <= 0 ? 0 : (l > G ? (int)G : (int)l);
        }
    }
    const int P2 = pow2_ceil(nc < 2 ? 2 : nc);
    const float* qrow = q + i * ldq;
    const float sq = qq[i];
    for (int t = threadIdx.x; t < P2; t += blockDim.x) {
        float d = __builtin_inff();
        int j = 0x7fffffff;
        if (t < nc) {
            j = si[t];
            // the distance kernel's bits: fma(-2, chain, s_q + s_g) (distance.h dm_value)
            d = __builtin_fmaf(-2.0f, dot_chain(qrow, g + (int64_t)j * ldg, D, vec), sq + gg[j]);
            if (!(d <= tv && key_less(d, j, tv, ti))) {  // not admissible under the bound
                d = __builtin_inff();
                j = 0x7fffffff;
            }
        }
        sv[t] = d;
        si[t] = j;
    }
    __syncthreads();
    bitonic_sort_kv(sv, si, P2);  // ascending (d, item)
    for (int t = threadIdx.x; t < K; t += blockDim.x) {
        const bool in = t < nc && si[t] != 0x7fffffff;
        out_idx[i * ldo + t] = in ? si[t] : -1;
        if (out_dist) out_dist[i * ldo + t] = in ? sv[t] : __builtin_inff();
    }
    if (threadIdx.x == 0) {
        need[i] = 0;
        atomicAdd(&st->rescored, (unsigned long long)nc);
    }
}

__global__ void sp_stats_kernel(const SpState* __restrict__ st, int32_t* __restrict__ stats) {
    stats[0] = st->need_rows;
    stats[1] = st->max_survivors;
    stats[2] = st->rescored < 0x7fffffffull ? (int32_t)st->rescored : 0x7fffffff;
    stats[3] = st->range_ok ? 0 : 1;
}

// The call's sizes and its workspace layout, pure functions of the shapes.  Workspace (bytes from
// the base, every part 256-byte aligned):
//   state                     SpState
//   qq [Q], gg [G]            squared norms (the distance kernels' rows_sqnorm)
//   qn [Q], gn [G]            norms = sqrt of those
//   sqn_s, nrm_s [ns]         the sample's gg / gn
//   colrec [Gp] float4        the survivor epilogue's column records (s_j, n_j, 0, 0)
//   tiles [pass / 256 x Gp / 256] int32   the rectangular tile list of one pass
//   per pass of `pass` rows:  hs [pass][ns] fp32 (sample bounds), list [pass][RR_SV_CAP] int2,
//                             cnt [pass] int32, wrow [pass], trow [pass] fp32, meta [pass] float4
//   q16 [Qp][Dp], g16 [Gp][Dp]   fp16 copies, zero-padded to the GEMM tile (Qp, Gp multiples of 256,
//                             Dp of 64)
// pass = the rows whose per-pass state fits SP_PASS_BYTES (whole 256-row tiles, at least one, at most
// 65536 rows), capped by Qp: no term grows with Q x G.
struct SpPlan {
    int S;
    int64_t ns, Qp, Gp, Dp, pass;
    int64_t o_qq, o_gg, o_qn, o_gn, o_sqs, o_nrs, o_colrec, o_tiles, o_hs, o_list, o_cnt, o_wrow, o_trow, o_meta, o_q16,
        o_g16, bytes;
};

static bool sp_plan(int64_t Q, int64_t G, int64_t D, int k, int sample_stride, SpPlan* p) {
    if (Q < 0 || Q >= (1ll << 31) || G <= 0 || G >= 0x7fffffff || D <= 0 || D > (1 << 20) || k < 1 || k > SP_K_MAX ||
        k > G || sample_stride < 0 || sample_stride == 1)
        return false;
    p->S = sample_stride == 0 ? RR_SAMPLE_STRIDE : sample_stride;
    p->ns = rr_sv_ns(G, p->S);
    p->Dp = (D + 63) / 64 * 64;
    p->Gp = (G + 255) / 256 * 256;
    p->Qp = (Q + 255) / 256 * 256;
    // rr_sv_pass_rows' rule: the persistent tile's two K-steps, a whole sample tile, 4 k sample items
    if (p->Dp < 128 || p->ns < 256 || p->ns < 4 * (int64_t)k || p->Gp / 256 > 65536) return false;
    const int64_t row_bytes = 4 * p->ns + 8 * (int64_t)RR_SV_CAP + 4 + 4 + 4 + 16;
    int64_t pass = SP_PASS_BYTES / row_bytes / 256 * 256;
    pass = pass < 256 ? 256 : pass > 65536 ? 65536 : pass;
    p->pass = pass < p->Qp || p->Qp == 0 ? pass : p->Qp;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += (bytes + 255) / 256 * 256;
        return at;
    };
    take(sizeof(SpState));
    p->o_qq = take(4 * Q);
    p->o_gg = take(4 * G);
    p->o_qn = take(4 * Q);
    p->o_gn = take(4 * G);
    p->o_sqs = take(4 * p->ns);
    p->o_nrs = take(4 * p->ns);
    p->o_colrec = take(16 * p->Gp);
    p->o_tiles = take(4 * (p->pass / 256) * (p->Gp / 256));
    p->o_hs = take(4 * p->pass * p->ns);
    p->o_list = take(8 * p->pass * (int64_t)RR_SV_CAP);
    p->o_cnt = take(4 * p->pass);
    p->o_wrow = take(4 * p->pass);
    p->o_trow = take(4 * p->pass);
    p->o_meta = take(16 * p->pass);
    p->o_q16 = take(2 * p->Qp * p->Dp);
    p->o_g16 = take(2 * p->Gp * p->Dp);
    p->bytes = o;
    return true;
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_search_prefilter_applies(int64_t Q, int64_t G, int64_t D, int k, int sample_stride) {
    SpPlan p;
    return sp_plan(Q, G, D, k, sample_stride, &p) ? 1 : 0;
}

REIDMI_API int64_t reidmi_search_prefiltered_workspace_bytes(int64_t Q, int64_t G, int64_t D, int k,
                                                             int sample_stride) {
    SpPlan p;
    return sp_plan(Q, G, D, k, sample_stride, &p) ? p.bytes : -1;
}

static int search_prefiltered_impl(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                   int64_t D, int k, const int64_t* q_pids, const int64_t* q_cams,
                                   const int64_t* g_pids, const int64_t* g_cams, const reidmi_search_filter* filter,
                                   const float* bound_dist, const int32_t* bound_idx, int64_t ldb, int64_t index_base,
                                   int32_t* out_idx, float* out_dist, int64_t ldo, int sample_stride, int32_t* need,
                                   int32_t* stats, void* ws, int64_t ws_bytes, void* stream) {
    // reidmi_search_bounded_f32's refusals (search.hip search_impl), then this call's own
    RM_REQUIRE(Q >= 0 && G > 0 && G < 0x7fffffff && D > 0 && ldq >= D && ldg >= D, "search: bad shape");
    RM_REQUIRE(k >= 1 && k <= G, "search: need 1 <= k <= G");
    RM_REQUIRE(k <= SP_K_MAX,
               "search: k > 128 is not fused; use reidmi_distmat_f32 + reidmi_topk_rows_f32 for larger k");
    RM_REQUIRE(out_idx != nullptr && ldo >= k, "search: out_idx required, ldo >= k");
    SrFilter flt;
    RM_TRY(sr_filter_make(q_pids, q_cams, g_pids, g_cams, filter, &flt));
    RM_REQUIRE(bound_dist != nullptr || bound_idx == nullptr, "search: bound_idx needs bound_dist");
    RM_REQUIRE(ldb >= 1, "search: need ldb >= 1");
    RM_REQUIRE(index_base >= 0 && index_base + G <= 0x7fffffff,
               "search: need index_base >= 0 and index_base + G <= 2^31 - 1");
    RM_REQUIRE(need != nullptr, "search_prefiltered: need required");
    RM_REQUIRE(sample_stride == 0 || sample_stride >= 2, "search_prefiltered: sample_stride is 0 (default) or >= 2");
    SpPlan p;
    RM_REQUIRE(sp_plan(Q, G, D, k, sample_stride, &p),
               "search_prefiltered: the pre-filter does not apply to this shape (reidmi_search_prefilter_applies)");
    RM_REQUIRE(ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= p.bytes,
               "search_prefiltered: workspace (reidmi_search_prefiltered_workspace_bytes, 16-byte aligned) required");
    if (Q == 0) return OK;
    RM_REQUIRE(q != nullptr && g != nullptr, "search: features required");
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    SpState* st = (SpState*)base;
    float *qq = (float*)(base + p.o_qq), *gg = (float*)(base + p.o_gg), *qn = (float*)(base + p.o_qn),
          *gn = (float*)(base + p.o_gn), *sqn_s = (float*)(base + p.o_sqs), *nrm_s = (float*)(base + p.o_nrs);
    float4* colrec = (float4*)(base + p.o_colrec);
    int* tiles = (int*)(base + p.o_tiles);
    float* hs = (float*)(base + p.o_hs);
    int2* list = (int2*)(base + p.o_list);
    int32_t* cnt = (int32_t*)(base + p.o_cnt);
    float *wrow = (float*)(base + p.o_wrow), *trow = (float*)(base + p.o_trow);
    float4* meta = (float4*)(base + p.o_meta);
    _Float16 *q16 = (_Float16*)(base + p.o_q16), *g16 = (_Float16*)(base + p.o_g16);
    const int T = (int)(p.Gp / 256);

    hipLaunchKernelGGL(sp_init_kernel, dim3(1), dim3(1), 0, s, st);
    RM_LAUNCHED();
    rows_sqnorm_launch(q, Q, D, ldq, qq, s);
    RM_LAUNCHED();
    rows_sqnorm_launch(g, G, D, ldg, gg, s);
    RM_LAUNCHED();
    hipLaunchKernelGGL(sp_sqrt_kernel, dim3((unsigned)ceil_div(Q, 256)), dim3(256), 0, s, qq, Q, qn);
    RM_LAUNCHED();
    hipLaunchKernelGGL(sp_sqrt_kernel, dim3((unsigned)ceil_div(G, 256)), dim3(256), 0, s, gg, G, gn);
    RM_LAUNCHED();
    RM_TRY(norm_max_launch(gg, gn, G, st->nmax2, s));
    RM_TRY(feat16_launch(q, Q, D, ldq, q16, p.Qp, p.Dp, &st->range_ok, s));
    RM_TRY(feat16_launch(g, G, D, ldg, g16, p.Gp, p.Dp, &st->range_ok, s));
    RM_TRY(rr_gather_norms_launch(gg, gn, p.ns, p.S, sqn_s, nrm_s, s));
    RM_TRY(rr_colrec_launch(gg, gn, G, p.Gp, colrec, s));

    float c[3];
    rank_select_consts((int)D, c);
    const SpBound bnd{bound_dist, bound_idx, ldb, index_base};
    const bool vec = (((uintptr_t)q | (uintptr_t)g) & 15) == 0 && (ldq & 3) == 0 && (ldg & 3) == 0;
    int tm_listed = -1;
    for (int64_t a = 0; a < Q; a += p.pass) {
        const int64_t nb = Q - a < p.pass ? Q - a : p.pass;
        const int tm = ceil_div(nb, 256);
        if (tm != tm_listed) {
            RM_TRY(rr_rect_tiles_launch(tm, T, tiles, s));
            tm_listed = tm;
        }
        // (a) the sample: W rows = every S-th gallery item (row pitch S * Dp)
        RM_TRY(rr_hi_sample_launch(q16 + a * p.Dp, p.Dp, g16, (int64_t)p.S * p.Dp, qq, qn, a, nb, sqn_s, nrm_s, p.ns, D,
                                   hs, s));
        hipLaunchKernelGGL(sp_threshold_kernel, dim3((unsigned)nb), dim3(256), 0, s, hs, p.ns, p.S, qq, qn, st, a, k,
                           c[0], c[1], c[2], flt, bnd, meta, wrow, trow, cnt, RR_SV_CAP);
        RM_LAUNCHED();
        RM_TRY(rr_survivors_launch(q16 + a * p.Dp, g16, p.Dp, p.Gp, G, D, nb, meta, colrec, tiles, (int64_t)tm * T,
                                   false, cnt, list, RR_SV_CAP, s));
        hipLaunchKernelGGL(sp_select_kernel, dim3((unsigned)nb), dim3(256), 0, s, cnt, list, RR_SV_CAP, wrow, trow, q,
                           ldq, g, ldg, (int)D, vec, qq, gg, a, G, k, flt, bnd, st, out_idx, out_dist, ldo, need);
        RM_LAUNCHED();
    }
    if (stats != nullptr) {
        hipLaunchKernelGGL(sp_stats_kernel, dim3(1), dim3(1), 0, s, st, stats);
        RM_LAUNCHED();
    }
    return OK;
}

REIDMI_API int reidmi_search_prefiltered_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G,
                                             int64_t ldg, int64_t D, int k, const int64_t* q_pids,
                                             const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                                             const float* bound_dist, const int32_t* bound_idx, int64_t ldb,
                                             int64_t index_base, int32_t* out_idx, float* out_dist, int64_t ldo,
                                             int sample_stride, int32_t* need, int32_t* stats, void* ws,
                                             int64_t ws_bytes, void* stream) {
    return search_prefiltered_impl(q, Q, ldq, g, G, ldg, D, k, q_pids, q_cams, g_pids, g_cams, nullptr, bound_dist,
                                   bound_idx, ldb, index_base, out_idx, out_dist, ldo, sample_stride, need, stats, ws,
                                   ws_bytes, stream);
}

REIDMI_API int reidmi_search_prefiltered_filtered_f32(
    const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg, int64_t D, int k,
    const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
    const reidmi_search_filter* flt, const float* bound_dist, const int32_t* bound_idx, int64_t ldb, int64_t index_base,
    int32_t* out_idx, float* out_dist, int64_t ldo, int sample_stride, int32_t* need, int32_t* stats, void* ws,
    int64_t ws_bytes, void* stream) {
    return search_prefiltered_impl(q, Q, ldq, g, G, ldg, D, k, q_pids, q_cams, g_pids, g_cams, flt, bound_dist,
                                   bound_idx, ldb, index_base, out_idx, out_dist, ldo, sample_stride, need, stats, ws,
                                   ws_bytes, stream);
}
