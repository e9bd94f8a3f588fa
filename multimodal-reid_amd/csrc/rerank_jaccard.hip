// rerank_jaccard.hip — R6+R7 of the k-reciprocal re-rank (stage map: rerank.hip): Jaccard with
// sequential fp16 sums, blended with od, for the columns [Q, N) (reranking.py:84-100), on gfx950.
//
//   jaccard_bounds_kernel   chunk boundaries of every sorted inverted list, once per call
//   jaccard_kernel<false>   the matrix form over sorted lists (reidmi_rr_jaccard_rows)
//   jaccard_kernel<true>    the selecting form: a chunk's first k in argsort order, then
//     + jaccard_merge_kernel  one merge per query (reidmi_rr_jaccard_topk_rows)
//   jaccard_scan_kernel     the matrix form over unsorted lists (the one-call driver, through
//                           jaccard_scan_launch of rerank.h)
// Boundary: from V_qe and its inverted index to final distances or rank lists.  JCH (rerank.h) is
// read only here: the kernels' chunk and every grid and byte count derived from it.
#include "backend.h"
#include "rerank.h"
#include "select.h"

namespace reidmi {

// ----------------------------------------------------------- R6 + R7: Jaccard
// One workgroup per (query i = q0 + blockIdx.y, chunk of gallery columns).  temp_min[r]
// (fp16 bits) lives in LDS; the nonzero columns c of V_qe[i] are visited in ascending order
// and each column's inverted list (rows ascending) updates distinct rows, so one barrier per
// column keeps every temp_min[r] a sequential fp16 sum in ascending c (reranking.py:90-92);
// the chunk's sub-range of each list is found by binary search.  Epilogue: Jaccard in fp16
// (reranking.py:93), blend with od in fp32 (reranking.py:95), write final[blockIdx.y][r-Q].
// od of (i, r) = OD[blockIdx.y * ld + (r - odc0)] / rowdiv[i].
// Chunk boundaries of every column's sorted row list, once per call: cbnd[c * (nch + 1) + b]
// = first position p in [off[c], off[c+1]) with irow[p] >= Q + b * JCH (b = nch: off[c+1]).
// jaccard_kernel then reads its slice with two loads instead of two binary searches per
// (query row, column) — those searches were a serial chain of dependent loads.
__global__ __launch_bounds__(256) void jaccard_bounds_kernel(const int64_t* __restrict__ off,
                                                             const int32_t* __restrict__ irow, int64_t N, int64_t Q,
                                                             int nch, int64_t* __restrict__ cbnd) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * (nch + 1)) return;
    const int64_t c = t / (nch + 1);
    const int b = (int)(t - c * (nch + 1));
    int64_t lo = off[c], hi = off[c + 1];
    if (b < nch) {
        const int64_t key = Q + (int64_t)b * JCH;
        while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (irow[m] < key) lo = m + 1; else hi = m; }
    } else {
        lo = hi;  // every row index is < N
    }
    cbnd[t] = lo;
}

// One final distance: tm = temp_min's fp16 bits, od the unscaled original distance, dv the query's
// od divisor, lam = fp32 of the fp16 (1 - lambda).  Jaccard in fp16 (every op rounded,
// reranking.py:93), the blend in fp32 (reranking.py:95).  The one definition for every Jaccard
// kernel, matrix or selecting form.
__device__ __forceinline__ float jaccard_blend_one(uint16_t tm, float od, float dv, float lam, float lam_f) {
    const float tv = h2f_bits(tm);
    const uint16_t den = f2h_bits(2.0f - tv);
    const uint16_t qt = f2h_bits(tv / h2f_bits(den));
    const uint16_t jac = f2h_bits(1.0f - h2f_bits(qt));
    const float a = h2f_bits(f2h_bits(h2f_bits(jac) * lam));
    const float b = (od / dv) * lam_f;
    return a + b;
}

// The epilogue of the matrix forms for one (query, chunk): tmin[t] (fp16 bits in LDS) is temp_min
// of chunk column t, od[t] its unscaled original distance.
__device__ __forceinline__ void jaccard_blend(const uint16_t* tmin, int span, const float* __restrict__ od, float dv,
                                              uint16_t lam16, float lam_f, float* __restrict__ out) {
    const float lam = h2f_bits(lam16);
    for (int t = threadIdx.x; t < span; t += blockDim.x) out[t] = jaccard_blend_one(tmin[t], od[t], dv, lam, lam_f);
}

// jaccard_kernel<false> is the matrix form above.  jaccard_kernel<true> is the selecting form
// (reidmi_rr_jaccard_topk_rows): the same walk and the same per-element blend, but the chunk's
// final distances are never stored (out / ldo unused).  The workgroup selects the K smallest
// (value, gallery index) of its chunk (topk_row_dev; within a chunk the order by chunk column is
// the order by gallery index) among the columns the label predicate keeps (evaluate.py:46-48:
// not the query's own pid and camera), and writes them as a sorted partial list
// part[(blockIdx.y * chunks + chunk) * K + 0..K), padded with (+inf, -1); entries carry the
// gallery index.  jaccard_merge_kernel joins a query's lists.  LDS: the matrix form's 20 KB +
// TkLds = 36.9 KB, four workgroups per CU (the matrix form: eight).
// The selecting form's extra arguments: the list length, the label arrays (all null: every column
// is kept) and the partial lists.  The matrix form's are empty, and last, so that its
// instantiation compiles to the code it had as a plain kernel.
template <bool SELECT>
struct JcSelect {};
template <>
struct JcSelect<true> {
    int K;
    const int64_t *qp, *qc, *gp, *gc;
    float2* part;
};

template <bool SELECT>
__global__ __launch_bounds__(256) void jaccard_kernel(const float* __restrict__ OD, int64_t ld, int64_t odc0,
                                                      const float* __restrict__ rowdiv, int64_t q0, int64_t Q,
                                                      int64_t N, Rows Vq, const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ irow, const uint16_t* __restrict__ ival,
                                                      const int64_t* __restrict__ cbnd, uint16_t lam16, float lam_f,
                                                      float* __restrict__ out, int64_t ldo, JcSelect<SELECT> sel) {
    __shared__ uint16_t tmin[JCH];
    const int64_t y = blockIdx.y;
    const int64_t i = q0 + y;
    const int64_t base = Q + (int64_t)blockIdx.x * JCH;
    const int64_t end = base + JCH < N ? base + JCH : N;
    const int span = (int)(end - base);
    for (int t = threadIdx.x; t < span; t += blockDim.x) tmin[t] = 0;
    __syncthreads();
    const int nz = Vq.len(i);
    const int64_t qb = Vq.beg(i);
    const int nb1 = (int)gridDim.x + 1;
    // V_qe[i]'s columns in batches of 256: each thread fetches one column's value and slice
    // bounds (jaccard_bounds_kernel) at once, so the column walk below has no dependent
    // bound loads; a thread's element of the next column's slice is loaded before the
    // barrier of the current one
    __shared__ int64_t s_p0[256];
    __shared__ int s_n[256];
    __shared__ float s_vi[256];
    for (int e0 = 0; e0 < nz; e0 += 256) {
        const int m = nz - e0 < 256 ? nz - e0 : 256;
        if ((int)threadIdx.x < m) {
            const int32_t c = Vq.col[qb + e0 + threadIdx.x];
            const int64_t p0 = cbnd[(int64_t)c * nb1 + blockIdx.x], p1 = cbnd[(int64_t)c * nb1 + blockIdx.x + 1];
            s_p0[threadIdx.x] = p0;
            s_n[threadIdx.x] = (int)(p1 - p0);
            s_vi[threadIdx.x] = h2f_bits(Vq.val[qb + e0 + threadIdx.x]);
        }
        __syncthreads();
        int nk = -1;
        float nv = 0.0f;
        auto fetch = [&](int e) {
            nk = -1;
            if ((int)threadIdx.x < s_n[e]) {
                const int64_t p = s_p0[e] + threadIdx.x;
                nk = (int)(irow[p] - base);
                nv = h2f_bits(ival[p]);
            }
        };
        fetch(0);
        for (int e = 0; e < m; e++) {
            const int k = nk;
            const float vr = nv;
            const float vi = s_vi[e];
            const int n = s_n[e];
            if (e + 1 < m) fetch(e + 1);
            if (k >= 0) {
                const float mn = vr < vi ? vr : vi;
                tmin[k] = f2h_bits(h2f_bits(tmin[k]) + mn);
            }
            for (int64_t p = s_p0[e] + 256 + threadIdx.x; p < s_p0[e] + n; p += blockDim.x) {  // long slices
                const int kk = (int)(irow[p] - base);
                const float vr2 = h2f_bits(ival[p]);
                const float mn = vr2 < vi ? vr2 : vi;
                tmin[kk] = f2h_bits(h2f_bits(tmin[kk]) + mn);
            }
            __syncthreads();
        }
    }
    if constexpr (!SELECT) {
        jaccard_blend(tmin, span, OD + y * ld + (base - odc0), rowdiv[i], lam16, lam_f, out + y * ldo + (base - Q));
    } else {
        __shared__ TkLds L;
        const float* __restrict__ od = OD + y * ld + (base - odc0);
        const float dv = rowdiv[i], lam = h2f_bits(lam16);
        const int64_t g0 = base - Q;  // gallery index of chunk column 0
        auto val = [&](int64_t t) { return jaccard_blend_one(tmin[t], od[t], dv, lam, lam_f); };
        if (sel.qp) {
            const int64_t qp = sel.qp[i], qc = sel.qc[i];
            topk_row_dev(val, span, sel.K, L,
                         [&](float, int t) { return !(sel.gp[g0 + t] == qp && sel.gc[g0 + t] == qc); });
        } else {
            topk_row_dev(val, span, sel.K, L);
        }
        const int n = L.s_nsel;
        float2* __restrict__ dst = sel.part + (y * gridDim.x + blockIdx.x) * (int64_t)sel.K;
        for (int t = threadIdx.x; t < sel.K; t += blockDim.x)
            dst[t] = t < n ? make_float2(L.sv[t], __int_as_float((int)(g0 + L.si[t])))
                           : make_float2(__builtin_inff(), __int_as_float(-1));
    }
}

// One workgroup per query row of the pass: joins the row's `chunks` partial lists (topk_merge_dev).
__global__ __launch_bounds__(256) void jaccard_merge_kernel(const float2* __restrict__ part, int chunks, int K,
                                                            int32_t* __restrict__ out_idx,
                                                            float* __restrict__ out_dist, int64_t ldo) {
    __shared__ TkLds L;
    const int64_t y = blockIdx.x;
    const float2* __restrict__ mine = part + y * chunks * (int64_t)K;
    topk_merge_dev([&](int64_t p) { return mine[p]; }, (int64_t)chunks * K, K, L, out_idx + y * ldo,
                   out_dist ? out_dist + y * ldo : nullptr);
}

// Jaccard over unsorted inverted lists: every chunk scans whole lists and filters rows.
__global__ __launch_bounds__(256) void jaccard_scan_kernel(const float* __restrict__ OD, int64_t ld,
                                                           const float* __restrict__ rowdiv, int64_t Q, int64_t N,
                                                           Rows Vq, const int64_t* __restrict__ off,
                                                           const int32_t* __restrict__ irow,
                                                           const uint16_t* __restrict__ ival, uint16_t lam16,
                                                           float lam_f, float* __restrict__ out, int64_t ldo) {
    __shared__ uint16_t tmin[JCH];
    const int64_t i = blockIdx.y;
    const int64_t base = Q + (int64_t)blockIdx.x * JCH;
    const int64_t end = base + JCH < N ? base + JCH : N;
    const int span = (int)(end - base);
    for (int t = threadIdx.x; t < span; t += blockDim.x) tmin[t] = 0;
    __syncthreads();
    const int nz = Vq.len(i);
    const int64_t qb = Vq.beg(i);
    for (int e = 0; e < nz; e++) {
        const int32_t c = Vq.col[qb + e];
        const float vi = h2f_bits(Vq.val[qb + e]);
        const int64_t p0 = off[c], p1 = off[c + 1];
        for (int64_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
            const int64_t r = irow[p];
            if (r < base || r >= end) continue;
            const float vr = h2f_bits(ival[p]);
            const float mn = vr < vi ? vr : vi;
            const int k = (int)(r - base);
            tmin[k] = f2h_bits(h2f_bits(tmin[k]) + mn);
        }
        __syncthreads();
    }
    jaccard_blend(tmin, span, OD + i * ld + base, rowdiv[i], lam16, lam_f, out + i * ldo + (base - Q));
}

int jaccard_scan_launch(const float* OD, int64_t ld, const float* rowdiv, int64_t Q, int64_t N, const Rows& Vq,
                        const int64_t* off, const int32_t* irow, const uint16_t* ival, uint16_t lam16, float lam_f,
                        float* out, int64_t ldo, hipStream_t s) {
    const int64_t G = N - Q;
    if (Q > 0 && G > 0) {
        dim3 grid(ceil_div(G, JCH), (unsigned)Q);
        hipLaunchKernelGGL(jaccard_scan_kernel, grid, dim3(256), 0, s, OD, ld, rowdiv, Q, N, Vq, off, irow, ival, lam16,
                           lam_f, out, ldo);
        RM_LAUNCHED();
    }
    return OK;
}

// bytes of the per-column chunk bounds of reidmi_rr_jaccard_rows (int64 per column and chunk
// boundary)
static int64_t jaccard_bounds_bytes(int64_t N, int64_t G) {
    const int64_t nch = (G + JCH - 1) / JCH;
    return N * (nch + 1) * 8;
}

// Partial lists of one row pass of reidmi_rr_jaccard_topk_rows: k (value, index) pairs per
// (query row of the pass, chunk).  -1 on arguments the call itself refuses.
constexpr int JT_K_MAX = 128;
static int64_t jaccard_topk_ws_bytes(int64_t rows, int64_t G, int k) {
    if (rows < 1 || rows > 65535 || G < 1 || G >= 0x7fffffff || k < 1 || k > JT_K_MAX || k > G) return -1;
    return rows * ((G + JCH - 1) / JCH) * k * 8;
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int64_t reidmi_rr_jaccard_bounds_bytes(int64_t N, int64_t G) {
    return N > 0 && G > 0 ? jaccard_bounds_bytes(N, G) : -1;
}

REIDMI_API int reidmi_rr_jaccard_rows(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn,
                                      const float* rowmax, int64_t Q, int64_t qlo, int64_t qhi, const int64_t* qoff,
                                      const int32_t* qcol, const uint16_t* qval, const int64_t* coff,
                                      const int32_t* irow, const uint16_t* ival, uint16_t one_minus_lambda_h,
                                      float lambda_f, float* out, int64_t ldo, float* chunk, int64_t chunk_rows,
                                      void* bounds, int64_t bounds_bytes, void* stream) {
    const int64_t G = N - Q;
    RM_REQUIRE(N > 0 && D > 0 && ldf >= D && 0 <= qlo && qlo <= qhi && qhi <= Q && Q <= N && ldo >= G &&
                   chunk_rows > 0 && chunk_rows <= 65535,
               "rr_jaccard_rows: bad arguments");
    if (qhi == qlo || G == 0) return OK;
    hipStream_t s = (hipStream_t)stream;
    const Rows Vq = csr_rows(qoff, qcol, qval);
    const int nch = ceil_div(G, JCH);
    RM_REQUIRE(bounds && ((uintptr_t)bounds & 7) == 0 && bounds_bytes >= jaccard_bounds_bytes(N, G),
               "rr_jaccard_rows: bounds of reidmi_rr_jaccard_bounds_bytes(N, N-Q) bytes (8-byte aligned) required");
    int64_t* cbnd = (int64_t*)bounds;
    hipLaunchKernelGGL(jaccard_bounds_kernel, dim3(ceil_div(N * (nch + 1), 256)), dim3(256), 0, s, coff, irow, N, Q,
                       nch, cbnd);
    RM_LAUNCHED();
    int rc;
    for (int64_t a = qlo; a < qhi; a += chunk_rows) {
        const int64_t nb = qhi - a < chunk_rows ? qhi - a : chunk_rows;
        // original_dist[a:a+nb, Q:N] (chunk, ld G)
        if ((rc = distmat_pre_launch(feat + a * ldf, nb, ldf, feat + Q * ldf, G, ldf, D, sqn + a, sqn + Q, chunk, G, s)))
            return rc;
        dim3 grid(ceil_div(G, JCH), (unsigned)nb);
        hipLaunchKernelGGL(jaccard_kernel<false>, grid, dim3(256), 0, s, (const float*)chunk, G, Q, rowmax, a, Q, N, Vq,
                           coff, irow, ival, (const int64_t*)cbnd, one_minus_lambda_h, lambda_f, out + (a - qlo) * ldo,
                           ldo, JcSelect<false>{});
        RM_LAUNCHED();
    }
    return OK;
}

REIDMI_API int64_t reidmi_rr_jaccard_topk_workspace_bytes(int64_t rows_per_pass, int64_t G, int k) {
    return jaccard_topk_ws_bytes(rows_per_pass, G, k);
}

// reidmi_rr_jaccard_rows with the selection in the Jaccard kernel: per row pass, the chunk's od
// rows, one sorted partial list per (query, chunk) (jaccard_kernel<true>), one merge per query
// (jaccard_merge_kernel).  The passes reuse ws in stream order.
REIDMI_API int reidmi_rr_jaccard_topk_rows(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn,
                                           const float* rowmax, int64_t Q, int64_t qlo, int64_t qhi,
                                           const int64_t* qoff, const int32_t* qcol, const uint16_t* qval,
                                           const int64_t* coff, const int32_t* irow, const uint16_t* ival,
                                           uint16_t one_minus_lambda_h, float lambda_f, int k, const int64_t* q_pids,
                                           const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                                           int32_t* out_idx, float* out_dist, int64_t ldo, float* chunk,
                                           int64_t chunk_rows, void* bounds, int64_t bounds_bytes, void* ws,
                                           int64_t ws_bytes, void* stream) {
    const int64_t G = N - Q;
    RM_REQUIRE(N > 0 && D > 0 && ldf >= D && 0 <= qlo && qlo <= qhi && qhi <= Q && Q <= N && G < 0x7fffffff,
               "rr_jaccard_topk_rows: bad shape or row range");
    RM_REQUIRE(k >= 1 && k <= G, "rr_jaccard_topk_rows: need 1 <= k <= G");
    RM_REQUIRE(k <= JT_K_MAX,
               "rr_jaccard_topk_rows: k > 128 is not fused; use reidmi_rr_jaccard_rows + reidmi_topk_rows_f32 for "
               "larger k");
    RM_REQUIRE(out_idx != nullptr && ldo >= k, "rr_jaccard_topk_rows: out_idx required, ldo >= k");
    const int nlab = (q_pids != nullptr) + (q_cams != nullptr) + (g_pids != nullptr) + (g_cams != nullptr);
    RM_REQUIRE(nlab == 0 || nlab == 4, "rr_jaccard_topk_rows: pass all four label arrays or none");
    RM_REQUIRE(chunk_rows > 0 && chunk_rows <= 65535, "rr_jaccard_topk_rows: need 1 <= chunk_rows <= 65535");
    RM_REQUIRE(ws != nullptr && ((uintptr_t)ws & 7) == 0 && ws_bytes >= jaccard_topk_ws_bytes(chunk_rows, G, k),
               "rr_jaccard_topk_rows: workspace (reidmi_rr_jaccard_topk_workspace_bytes(chunk_rows, N-Q, k), 8-byte "
               "aligned) required");
    RM_REQUIRE(bounds && ((uintptr_t)bounds & 7) == 0 && bounds_bytes >= jaccard_bounds_bytes(N, G),
               "rr_jaccard_topk_rows: bounds of reidmi_rr_jaccard_bounds_bytes(N, N-Q) bytes (8-byte aligned) required");
    if (qhi == qlo) return OK;
    RM_REQUIRE(feat && sqn && rowmax && qoff && coff && chunk, "rr_jaccard_topk_rows: inputs required");
    hipStream_t s = (hipStream_t)stream;
    const Rows Vq = csr_rows(qoff, qcol, qval);
    const int nch = ceil_div(G, JCH);
    int64_t* cbnd = (int64_t*)bounds;
    hipLaunchKernelGGL(jaccard_bounds_kernel, dim3(ceil_div(N * (nch + 1), 256)), dim3(256), 0, s, coff, irow, N, Q,
                       nch, cbnd);
    RM_LAUNCHED();
    const JcSelect<true> sel{k, q_pids, q_cams, g_pids, g_cams, (float2*)ws};
    const float2* part = sel.part;
    int rc;
    for (int64_t a = qlo; a < qhi; a += chunk_rows) {
        const int64_t nb = qhi - a < chunk_rows ? qhi - a : chunk_rows;
        // original_dist[a:a+nb, Q:N] (chunk, ld G)
        if ((rc = distmat_pre_launch(feat + a * ldf, nb, ldf, feat + Q * ldf, G, ldf, D, sqn + a, sqn + Q, chunk, G, s)))
            return rc;
        hipLaunchKernelGGL(jaccard_kernel<true>, dim3(nch, (unsigned)nb), dim3(256), 0, s, (const float*)chunk, G, Q,
                           rowmax, a, Q, N, Vq, coff, irow, ival, (const int64_t*)cbnd, one_minus_lambda_h, lambda_f,
                           (float*)nullptr, (int64_t)0, sel);
        RM_LAUNCHED();
        hipLaunchKernelGGL(jaccard_merge_kernel, dim3((unsigned)nb), dim3(256), 0, s, part, nch, k,
                           out_idx + (a - qlo) * ldo, out_dist ? out_dist + (a - qlo) * ldo : nullptr, ldo);
        RM_LAUNCHED();
    }
    return OK;
}
