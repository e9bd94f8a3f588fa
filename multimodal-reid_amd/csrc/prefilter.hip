// prefilter.hip — the fp16 pre-filter of the re-rank's initial_rank (R2) on gfx950: the rows of
// reranking.py:45-48 (od = D / rowmax, stable argsort, first K) selected from bounds of an fp16
// GEMM and recomputed exactly, in the dense (rank_select1_kernel) and the sampled survivor form
// (rr_sample_kernel, rank_select_sv_kernel), plus the fp16 feature copy and the norm maxima they
// need.  Called only from rerank_rank.hip (backend.h); the selection helpers are select.h's.
#include "backend.h"
#include "prefilter.h"
#include "select.h"

#include <cmath>

// RS_STATS (a printf of rank_select1_kernel's list sizes) is a tools-only diagnostic.  The guard
// names the tools define, so the build compiles this file for both libraries although it has no
// tools entry point: that second compile is accepted.
#if !defined(REIDMI_TOOLS) && defined(RS_STATS)
#error "prefilter.hip: RS_STATS builds only with -DREIDMI_TOOLS (never into libreidmi.so)"
#endif

namespace reidmi {

// ------------------------------------------------- re-rank R2 with an fp16 pre-filter
// The staged re-rank's initial_rank rows (reranking.py:45-48: od[i,:] = D[i,:] / max_j D[i,j]
// for the symmetric D, stable argsort, first K) without the exact N-wide distance row: the
// fp16 GEMM gives dot~_ij = x~_i . x~_j (x~ = fp16(x), fp32 accumulation) and
//   |d~_ij - d_ij| <= e_ij = 1.01 (c_rel n_i n_j + 2^-23 (s_i + s_j) + c_abs (n_i + n_j) + D 2^-49)
// with d~ = fma(-2, dot~, s_i + s_j), d the exact fp32 chain value (dist_exact, the distance
// kernel's bits), s = squared norms, n = sqrt(s), c_rel = 2 (2^-10 + 2^-22 + 2.02 D 2^-24) +
// 2.02 2^-23 (fp16 operand rounding 2^-11 relative + 2^-25 absolute per element, both
// accumulation chains, the final fma), c_abs = 2.01 2^-25 sqrt(D).  Then, with lo = d~ - e,
// hi = d~ + e:
//   * the K smallest (od, j) all satisfy d_j <= tau' = tau + |tau| 2^-21, tau = the K-th
//     smallest hi (K items have d <= hi <= tau; od = fl(d / r) is monotone and one rounding
//     cannot move a d above tau (1 + 2^-22) to an od at or below fl(tau / r)), and every such
//     item has lo <= d <= tau': the candidate set {j : lo_j <= tau'} contains them;
//   * the row max is attained among {j : hi_j >= max_k lo_k}.
// The candidates' exact distances then give the same rowmax and the same K indices as the
// full row, bit for bit.  Only hi reaches HBM (the GEMM's EPI_RRHI epilogue computes it from
// the product and the items' norms); the selection takes lo = hi - w_i with the row's width w_i
// >= hi_ij - lo_ij for every j (rr_width), which only widens both candidate sets.  A row whose
// candidate lists overflow, or with a non-finite bound or
// max, is marked in need[] for the exact rows (reranking.HipStages.rank_rows runs them through
// the exact distance kernel + selection).
// (dist_exact, block_max and rr_width: prefilter.h, shared with the pre-filtered search)

// Keep the entries j of idx[0, n) with keep(j) (order preserved, in place); one full wave.
template <typename KEEP>
__device__ int compact_wave(int* idx, int n, KEEP keep) {
    const int lane = threadIdx.x & 63;
    int w = 0;
    for (int b = 0; b < n; b += 64) {
        const int t = b + lane;
        const int j = t < n ? idx[t] : 0;
        const bool k = t < n && keep(j);
        const uint64_t m = __ballot(k);
        if (k) idx[w + __popcll(m & ((1ull << lane) - 1))] = j;
        w += __popcll(m);
    }
    return w;
}

// Rows of the k-reciprocal R2 from the pre-filter bounds hi ([rows][ldd] fp32, the EPI_RRHI
// GEMM epilogue: gemm.h rr_hi), lo = hi - w_i (rr_width): the K-th smallest hi bounds the K-th
// smallest exact distance, every item with lo <= that bound is a candidate of the top K, every
// item with hi >= the largest lo a candidate of the row max; both are recomputed exactly.
// One stream over the row feeds the K-smallest-hi selection and both candidate lists at once,
// against the running thresholds -- the running K-th smallest hi only decreases and the
// running max lo only increases, so each list holds a superset of the final one; a list near
// capacity, and both lists at the end, are filtered against the current thresholds (the exact
// set that three separate passes over the row give; that earlier kernel ran 0.116 s against
// 0.055 s on MSMT17's R2, DESIGN.md §4, and was removed with its RS_SINGLE_PASS switch).
constexpr int RS1_CHUNK = 1024;
// chunk of the stream, selection buffer, candidate and max-list capacities
constexpr int RS1_CH = RS1_CHUNK, RS1_TKCAP = 2 * RS1_CH, RS1_CCAP = 2 * RS1_CH, RS1_MCAP = RS1_CH + RS1_CH / 2;
struct Rs1Lds {
    float sv[RS1_TKCAP];
    int si[RS1_TKCAP];
    int s_cnt, s_nsel;
    float s_tv;
    int s_ti;
};

__global__ __launch_bounds__(256) void rank_select1_kernel(const float* __restrict__ dot, int64_t ldd,
                                                           const float* __restrict__ feat, int64_t ldf, int D,
                                                           const float* __restrict__ sqn,
                                                           const float* __restrict__ nrm, int64_t row0, int64_t N,
                                                           int K, float c_rel, float c_abs, float c_d,
                                                           const float* __restrict__ nmax2,
                                                           int32_t* __restrict__ rank_out,
                                                           float* __restrict__ rowmax_out, int32_t* __restrict__ need) {
    __shared__ Rs1Lds L;
    __shared__ int ci[RS1_CCAP];
    __shared__ int mi[RS1_MCAP];
    __shared__ int s_nc, s_nm, s_bad;
    __shared__ float red[4];
    const int64_t r = blockIdx.x, i = row0 + r;
    const float* drow = dot + r * ldd;   // the bounds hi of the row (EPI_RRHI)
    const float w = rr_width(sqn[i], nrm[i], nmax2[0], nmax2[1], c_rel, c_abs, c_d);
    const int wv = threadIdx.x >> 6;
    auto bounds_v = [&](float hj, float& lo, float& hi) {
        hi = hj;
        lo = hj - w;
    };
    auto bounds = [&](int64_t j, float& lo, float& hi) { bounds_v(drow[j], lo, hi); };
    // chunk loads (see the stream below): thread t takes items c0 + 4 (t + 256 u) .. + 3, one
    // 16-byte load each (ldd % 4 == 0; a vector that starts below N ends below ldd)
    constexpr int U = RS1_CH / 1024;
    auto load = [&](int64_t c0, float4* d) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = c0 + 4 * (u * 256 + threadIdx.x);
            d[u] = j < N ? *(const float4*)(drow + j) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto thr_of = [](float tau) { return tau + fabsf(tau) * 0x1p-21f + 1e-37f; };
    // the max-list threshold starts at the first chunk's largest lo
    float ml = -__builtin_inff();
    for (int64_t j = threadIdx.x; j < N && j < RS1_CH; j += blockDim.x) {
        float lo, hi;
        bounds(j, lo, hi);
        ml = fmaxf(ml, lo);
    }
    float mlo = block_max(ml, red);
    if (threadIdx.x == 0) { L.s_cnt = 0; L.s_nsel = 0; L.s_tv = __builtin_inff(); L.s_ti = 0x7fffffff; s_nc = 0; s_nm = 0; s_bad = 0; }
    __syncthreads();
    bool bad = false, c_lost = false, m_lost = false;
    float thr = __builtin_inff();
    // the chunk loads run three chunks ahead of the selection (four register sets in turn)
    auto chunk = [&](int64_t c0, const float4* cd) {
        const float tv = L.s_tv;
        const int ti = L.s_ti, nsel = L.s_nsel;
#pragma unroll
        for (int v = 0; v < 4 * U; v++) {
            const int64_t j = c0 + 4 * ((v >> 2) * 256 + threadIdx.x) + (v & 3);
            if (j < N) {
                float lo, hi;
                const float4 q = cd[v >> 2];
                bounds_v((v & 3) == 0 ? q.x : (v & 3) == 1 ? q.y : (v & 3) == 2 ? q.z : q.w, lo, hi);
                ml = fmaxf(ml, lo);
                bad = bad || !(lo == lo && hi == hi && hi < __builtin_inff());
                if (key_less(hi, (int)j, tv, ti)) {
                    const int p = atomicAdd(&L.s_cnt, 1);
                    L.sv[nsel + p] = hi;
                    L.si[nsel + p] = (int)j;
                }
                if (!c_lost && lo <= thr) ci[atomicAdd(&s_nc, 1)] = (int)j;
                if (!m_lost && hi >= mlo) mi[atomicAdd(&s_nm, 1)] = (int)j;
            }
        }
        const float wm = wave_max(ml);
        if ((threadIdx.x & 63) == 0) red[wv] = wm;
        __syncthreads();
        const bool last = c0 + RS1_CH >= N;
        const int n = L.s_nsel + L.s_cnt, nc = s_nc, nm = s_nm;
        mlo = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        __syncthreads();  // every thread has read the counters before anyone appends again
        // the selection is also merged before the candidate list is filtered, so that the
        // filter uses the current K-th bound (the selection buffer alone merges rarely)
        if (last || n > RS1_TKCAP - RS1_CH || (!c_lost && nc > RS1_CCAP - RS1_CH)) {
            const int P = pow2_ceil(n < 2 ? 2 : n);
            for (int t = n + threadIdx.x; t < P; t += blockDim.x) { L.sv[t] = __builtin_inff(); L.si[t] = 0x7fffffff; }
            __syncthreads();
            bitonic_sort_kv(L.sv, L.si, P);
            if (threadIdx.x == 0) {
                const int ns = n < K ? n : K;
                L.s_nsel = ns;
                L.s_cnt = 0;
                if (ns == K) { L.s_tv = L.sv[K - 1]; L.s_ti = L.si[K - 1]; }
            }
            __syncthreads();
        }
        if (L.s_nsel == K) thr = thr_of(L.s_tv);
        // filter the lists when the next chunk could overrun them, and at the end; a list
        // still too long afterwards is dropped and rebuilt by a second pass with the final
        // thresholds
        if (last || (!c_lost && nc > RS1_CCAP - RS1_CH) || (!m_lost && nm > RS1_MCAP - RS1_CH)) {
            if (wv == 0 && !c_lost) {
                const int k = compact_wave(ci, nc, [&](int j) {
                    float lo, hi;
                    bounds(j, lo, hi);
                    return lo <= thr;
                });
                if (threadIdx.x == 0) s_nc = k;
            } else if (wv == 1 && !m_lost) {
                const int k = compact_wave(mi, nm, [&](int j) {
                    float lo, hi;
                    bounds(j, lo, hi);
                    return hi >= mlo;
                });
                if (threadIdx.x == 64) s_nm = k;
            }
            __syncthreads();
            c_lost = c_lost || (!last && s_nc > RS1_CCAP - RS1_CH);
            m_lost = m_lost || (!last && s_nm > RS1_MCAP - RS1_CH);
            __syncthreads();  // every thread has read the counters before anyone appends again
        }
    };
    float4 xd[U], yd[U], zd[U], wd[U];
    load(0, xd);
    load(RS1_CH, yd);
    load(2 * RS1_CH, zd);
    for (int64_t c0 = 0; c0 < N; c0 += 4 * RS1_CH) {
        load(c0 + 3 * RS1_CH, wd);
        chunk(c0, xd);
        if (c0 + RS1_CH >= N) break;
        load(c0 + 4 * RS1_CH, xd);
        chunk(c0 + RS1_CH, yd);
        if (c0 + 2 * RS1_CH >= N) break;
        load(c0 + 5 * RS1_CH, yd);
        chunk(c0 + 2 * RS1_CH, zd);
        if (c0 + 3 * RS1_CH >= N) break;
        load(c0 + 6 * RS1_CH, zd);
        chunk(c0 + 3 * RS1_CH, wd);
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if ((c_lost || m_lost) && !s_bad) {  // uniform
        if (threadIdx.x == 0) {
            if (c_lost) s_nc = 0;
            if (m_lost) s_nm = 0;
        }
        __syncthreads();
        for (int64_t j = threadIdx.x; j < N; j += blockDim.x) {
            float lo, hi;
            bounds(j, lo, hi);
            if (c_lost && lo <= thr) {
                const int p = atomicAdd(&s_nc, 1);
                if (p < RS1_CCAP) ci[p] = (int)j;
            }
            if (m_lost && hi >= mlo) {
                const int p = atomicAdd(&s_nm, 1);
                if (p < RS1_MCAP) mi[p] = (int)j;
            }
        }
        __syncthreads();
    }
    const float tau = L.sv[K - 1];
    const int nc = s_nc, nm = s_nm;
#ifdef RS_STATS
    if (threadIdx.x == 0 && (blockIdx.x % 1024) == 7)
        printf("RS row %lld nc %d nm %d clost %d mlost %d bad %d\n", (long long)i, nc, nm, (int)c_lost, (int)m_lost, s_bad);
#endif
    bool exact = s_bad || !(tau <= 3.0e38f && tau >= -3.0e38f) || nc > RS1_TKCAP || nm > RS1_MCAP;  // the sort runs in the selection buffer
    float rmax = 0.0f;
    if (!exact) {
        float m = -__builtin_inff();
        for (int t = threadIdx.x; t < nm; t += blockDim.x) m = fmaxf(m, dist_exact(feat, ldf, D, sqn, i, mi[t]));
        rmax = block_max(m, red);
        exact = !(rmax > 0.0f && rmax < __builtin_inff());  // degenerate rows: the exact path
    }
    if (!exact) {
        float* cv = L.sv;  // the selection buffer is free once tau is read
        for (int t = threadIdx.x; t < nc; t += blockDim.x) cv[t] = dist_exact(feat, ldf, D, sqn, i, ci[t]) / rmax;
        const int P = pow2_ceil(nc < 2 ? 2 : nc);
        for (int t = nc + threadIdx.x; t < P; t += blockDim.x) { cv[t] = __builtin_inff(); ci[t] = 0x7fffffff; }
        __syncthreads();
        bitonic_sort_kv(cv, ci, P);
        for (int t = threadIdx.x; t < K; t += blockDim.x) rank_out[r * K + t] = ci[t];
        if (threadIdx.x == 0) {
            rowmax_out[r] = rmax;
            need[r] = 0;
        }
        return;
    }
    if (threadIdx.x == 0) need[r] = 1;
}

// The pair bound's constants for D-dimensional features (fp16-rounded operands, fp32 MFMA
// accumulation; the derivation is in the description of the bound above rank_select1_kernel).
void rank_select_consts(int D, float c[3]) {
    const double c_rel = 2.0 * (0x1p-10 + 0x1p-22 + 2.02 * D * 0x1p-24) + 2.02 * 0x1p-23;
    const double c_abs = 2.01 * 0x1p-25 * std::sqrt((double)D);
    const double c_d = D * 0x1p-49;
    c[0] = (float)(c_rel * (1.0 + 0x1p-20));
    c[1] = (float)(c_abs * (1.0 + 0x1p-20));
    c[2] = (float)(c_d * (1.0 + 0x1p-20));
}

// max over the items of the norms (out2[0]) and squared norms (out2[1]); fmaxf skips NaN (a NaN
// norm makes its bounds NaN, which sends the rows to the exact path)
__global__ __launch_bounds__(1024) void norm_max_kernel(const float* __restrict__ sqn, const float* __restrict__ nrm,
                                                        int64_t N, float* __restrict__ out2) {
    __shared__ float red[2][16];
    float a = 0.0f, b = 0.0f;
    for (int64_t j = threadIdx.x; j < N; j += blockDim.x) {
        a = fmaxf(a, nrm[j]);
        b = fmaxf(b, sqn[j]);
    }
    a = wave_max(a);
    b = wave_max(b);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++) {
            a = fmaxf(a, red[0][w]);
            b = fmaxf(b, red[1][w]);
        }
        out2[0] = a;
        out2[1] = b;
    }
}

int norm_max_launch(const float* sqn, const float* nrm, int64_t N, float* out2, hipStream_t s) {
    RM_REQUIRE(N > 0 && sqn && nrm && out2, "norm_max: bad arguments");
    hipLaunchKernelGGL(norm_max_kernel, dim3(1), dim3(1024), 0, s, sqn, nrm, N, out2);
    RM_LAUNCHED();
    return OK;
}

// rank_select1_kernel over rows [row0, row0 + rows) of the pre-filter bounds `dot` ([rows][ldd]
// fp32 hi, ldd >= N, the EPI_RRHI GEMM), nmax2 = norm_max_kernel's maxima.
int rank_select_launch(float* dot, int64_t ldd, const float* feat, int64_t ldf, int D, const float* sqn,
                       const float* nrm, const float* nmax2, int64_t row0, int64_t rows, int64_t N, int K,
                       int32_t* rank_out, float* rowmax_out, int32_t* need, hipStream_t s) {
    RM_REQUIRE(K >= 1 && K <= 64 && K <= N && ldd >= N && ldd % 4 == 0 && rows >= 0 && nmax2 &&
                   ((uintptr_t)dot & 15) == 0,
               "rank_select: bad arguments");
    if (rows == 0) return OK;
    float c[3];
    rank_select_consts(D, c);
    hipLaunchKernelGGL(rank_select1_kernel, dim3((unsigned)rows), dim3(256), 0, s, dot, ldd, feat, ldf, D, sqn, nrm,
                       row0, N, K, c[0], c[1], c[2], nmax2, rank_out, rowmax_out, need);
    RM_LAUNCHED();
    return OK;
}

// ------------------------------------------ R2 pre-filter with the selection in the GEMM
// The dense form above writes hi for every (row, item) pair and streams it back (N^2 fp32: 4 TB
// each way at N = 1M).  The sampled form keeps the selection's state out of HBM:
//  1. hi of each row against a sample of the items (every S-th item; EPI_RRHI, [rows][ns]);
//     rr_sample_kernel: U_r = the K-th smallest hi in the sample bounds tau_r (the K-th
//     smallest hi over all items) from above, and lb_r = max over the sample of lo = hi - w_r
//     bounds the row's largest lo from below;
//  2. the full GEMM with the EPI_RRSV epilogue appends to row r's list only the pairs with
//     hi <= hmax_r (every pair with lo <= thr(U_r)) or hi >= lb_r (gemm.h) -- a superset of both of rank_select1's final
//     candidate lists ({lo <= thr(tau)} and {hi >= max lo}), and it holds the K smallest hi
//     (hi <= tau <= U) and the largest hi (>= max lo >= lb): the list's K-th smallest hi is
//     tau itself and its largest hi the row's largest;
//  3. rank_select_sv_kernel: sorts the row's list by (hi, index), takes tau and max lo from it,
//     and runs rank_select1's exact tail (exact chain for both candidate lists, rowmax, stable
//     order by od = d / rowmax): the same rank_out / rowmax bits.
// A row whose list overflows RR_SV_CAP, holds a non-finite bound, or whose candidate lists
// exceed rank_select1's capacities is marked in need[] for the exact rows, as before.
__global__ __launch_bounds__(256) void rr_sample_kernel(const float* __restrict__ hs, int64_t lds, int64_t ns,
                                                        const float* __restrict__ sqn, const float* __restrict__ nrm,
                                                        const float* __restrict__ nmax2, int64_t row0, int K,
                                                        float c_rel, float c_abs, float c_d,
                                                        float4* __restrict__ meta, float* __restrict__ wrow,
                                                        int32_t* __restrict__ cnt, int cap) {
    __shared__ TkLds L;
    __shared__ float red[4];
    const int64_t r = blockIdx.x, i = row0 + r;
    const float* row = hs + r * lds;
    const float w = rr_width(sqn[i], nrm[i], nmax2[0], nmax2[1], c_rel, c_abs, c_d);
    float mx = -__builtin_inff();
    int bad = 0;
    for (int64_t j = threadIdx.x; j < ns; j += blockDim.x) {
        const float v = row[j];
        bad |= !(v < __builtin_inff());  // NaN or +inf
        mx = fmaxf(mx, v);
    }
    mx = block_max(mx, red);
    bad = __syncthreads_or(bad);
    topk_row_dev([&](int64_t j) { return row[j]; }, ns, K, L);
    if (threadIdx.x == 0) {
        const float U = L.sv[K - 1];
        const bool ok = !bad && ns >= K && U < 3.0e38f && U > -3.0e38f && mx < 3.0e38f;
        // the epilogue keeps a pair unless lb > hi > hmax: hmax bounds from above every hi whose
        // lo = fl(hi - w) is <= thr(U) (the widening covers the roundings of hi - w and of T + w)
        const float T = U + fabsf(U) * 0x1p-21f + 1e-37f;
        const float hmax = (T + w) + (fabsf(T) + w) * 0x1p-20f + 1e-37f;
        meta[r] = make_float4(sqn[i], nrm[i], hmax, mx - w);  // the survivor epilogue's row record
        wrow[r] = w;
        cnt[r] = ok ? 0 : cap + 1;
    }
}

__global__ __launch_bounds__(256) void rank_select_sv_kernel(const int32_t* __restrict__ cnt,
                                                             const int2* __restrict__ list, int cap,
                                                             const float* __restrict__ wrow,
                                                             const float* __restrict__ feat, int64_t ldf, int D,
                                                             const float* __restrict__ sqn, int64_t row0, int K,
                                                             int32_t* __restrict__ rank_out,
                                                             float* __restrict__ rowmax_out,
                                                             int32_t* __restrict__ need) {
    __shared__ float sv[RR_SV_CAP];
    __shared__ int si[RR_SV_CAP];
    __shared__ float red[4];
    __shared__ int s_nc, s_fm;
    const int64_t r = blockIdx.x, i = row0 + r;
    const int n = cnt[r];
    if (n > cap || n < K) {  // overflow, a non-finite bound, or (never for N >= K) too few
        if (threadIdx.x == 0) need[r] = 1;
        return;
    }
    const int2* lr = list + r * cap;
    const int P = pow2_ceil(n < 2 ? 2 : n);
    for (int t = threadIdx.x; t < P; t += blockDim.x) {
        if (t < n) {
            const int2 e = lr[t];
            sv[t] = __builtin_bit_cast(float, e.y);
            si[t] = e.x;
        } else {
            sv[t] = __builtin_inff();
            si[t] = 0x7fffffff;
        }
    }
    int bad = 0;
    for (int t = threadIdx.x; t < n; t += blockDim.x) bad |= !(sv[t] < __builtin_inff());  // NaN or +inf
    if (threadIdx.x == 0) { s_nc = 0; s_fm = n; }
    if (__syncthreads_or(bad)) {  // a non-finite bound: the exact path, as rank_select1
        if (threadIdx.x == 0) need[r] = 1;
        return;
    }
    bitonic_sort_kv(sv, si, P);  // ascending (hi, index)
    const float w = wrow[r];
    const float tau = sv[K - 1];
    const float th = tau + fabsf(tau) * 0x1p-21f + 1e-37f;  // rank_select1's thr_of
    const float mlo = sv[n - 1] - w;                         // the row's largest lo
    // candidate list = the prefix with lo = hi - w <= th; max list = the suffix with hi >= mlo
    int pc = 0, fm = n;
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        if (sv[t] - w <= th) pc = t + 1 > pc ? t + 1 : pc;
        if (sv[t] >= mlo) fm = t < fm ? t : fm;
    }
    atomicMax(&s_nc, pc);
    atomicMin(&s_fm, fm);
    __syncthreads();
    const int nc = s_nc, f0 = s_fm, nm = n - f0;
    bool exact = !(tau <= 3.0e38f && tau >= -3.0e38f) || nc > RS1_TKCAP || nm > RS1_MCAP;
    float rmax = 0.0f;
    if (!exact) {
        float m = -__builtin_inff();
        for (int t = f0 + threadIdx.x; t < n; t += blockDim.x) m = fmaxf(m, dist_exact(feat, ldf, D, sqn, i, si[t]));
        rmax = block_max(m, red);
        exact = !(rmax > 0.0f && rmax < __builtin_inff());  // degenerate rows: the exact path
    }
    if (!exact) {
        // the candidates are sv / si [0, nc): their exact od replaces the bound in place
        const int P2 = pow2_ceil(nc < 2 ? 2 : nc);
        __syncthreads();  // every thread is done reading sv / si [f0, n) above
        for (int t = threadIdx.x; t < P2; t += blockDim.x) {
            if (t < nc) {
                sv[t] = dist_exact(feat, ldf, D, sqn, i, si[t]) / rmax;
            } else {
                sv[t] = __builtin_inff();
                si[t] = 0x7fffffff;
            }
        }
        __syncthreads();
        bitonic_sort_kv(sv, si, P2);
        for (int t = threadIdx.x; t < K; t += blockDim.x) rank_out[r * K + t] = si[t];
        if (threadIdx.x == 0) {
            rowmax_out[r] = rmax;
            need[r] = 0;
        }
        return;
    }
    if (threadIdx.x == 0) need[r] = 1;
}

int rr_sample_launch(const float* hs, int64_t lds, int64_t ns, const float* sqn, const float* nrm, const float* nmax2,
                     int64_t row0, int64_t rows, int K, int D, float4* meta, float* wrow, int32_t* cnt, int cap,
                     hipStream_t s) {
    RM_REQUIRE(K >= 1 && K <= 64 && ns >= K && rows >= 0 && nmax2, "rr_sample: bad arguments");
    if (rows == 0) return OK;
    float c[3];
    rank_select_consts(D, c);
    hipLaunchKernelGGL(rr_sample_kernel, dim3((unsigned)rows), dim3(256), 0, s, hs, lds, ns, sqn, nrm, nmax2, row0, K,
                       c[0], c[1], c[2], meta, wrow, cnt, cap);
    RM_LAUNCHED();
    return OK;
}

int rank_select_sv_launch(const int32_t* cnt, const int2* list, int cap, const float* wrow, const float* feat,
                          int64_t ldf, int D, const float* sqn, int64_t row0, int64_t rows, int K, int32_t* rank_out,
                          float* rowmax_out, int32_t* need, hipStream_t s) {
    RM_REQUIRE(K >= 1 && K <= 64 && cap >= 1 && cap <= RR_SV_CAP && rows >= 0, "rank_select_sv: bad arguments");
    if (rows == 0) return OK;
    hipLaunchKernelGGL(rank_select_sv_kernel, dim3((unsigned)rows), dim3(256), 0, s, cnt, list, cap, wrow, feat, ldf, D,
                       sqn, row0, K, rank_out, rowmax_out, need);
    RM_LAUNCHED();
    return OK;
}

// fp16 copy of the features for the pre-filter GEMM: [Np][Dp], zero-padded rows / columns;
// *range_ok cleared when an element is beyond +-2^15 (fp16 would overflow) or not finite.
__global__ void feat16_kernel(const float* __restrict__ x, int64_t N, int64_t D, int64_t ldx, _Float16* __restrict__ y,
                              int64_t Np, int64_t Dp, int32_t* __restrict__ range_ok) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Np * Dp) return;
    const int64_t r = t / Dp, c = t - r * Dp;
    float v = 0.0f;
    if (r < N && c < D) {
        v = x[r * ldx + c];
        if (!(fabsf(v) <= 32768.0f)) { *range_ok = 0; v = 0.0f; }
    }
    y[t] = (_Float16)v;
}

int feat16_launch(const float* x, int64_t N, int64_t D, int64_t ldx, void* y, int64_t Np, int64_t Dp,
                  int32_t* range_ok, hipStream_t s) {
    RM_REQUIRE(N > 0 && D > 0 && ldx >= D && Np >= N && Dp >= D && range_ok, "feat16: bad arguments");
    hipLaunchKernelGGL(feat16_kernel, dim3((unsigned)ceil_div(Np * Dp, 256)), dim3(256), 0, s, x, N, D, ldx,
                       (_Float16*)y, Np, Dp, range_ok);
    RM_LAUNCHED();
    return OK;
}

}  // namespace reidmi
