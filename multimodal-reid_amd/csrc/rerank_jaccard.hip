// rerank_jaccard.hip — R6+R7 of the k-reciprocal re-rank (stage map: rerank.hip): Jaccard with
// sequential fp16 sums, blended with od, for the columns [Q, N) (reranking.py:84-100), on gfx950.
//
//   jaccard_bounds_kernel   chunk boundaries of every sorted inverted list, once per call
//   jaccard_kernel<false>   the matrix form over sorted lists (reidmi_rr_jaccard_rows)
//   jaccard_kernel<true>    the selecting form: a chunk's first k in argsort order, then
//     + jaccard_merge_kernel  one merge per query (reidmi_rr_jaccard_topk_rows)
//   jaccard_scan_kernel     the matrix form over unsorted lists (the one-call driver, through
//                           jaccard_scan_launch of rerank.h)
//   jaccard_self_kernel     the Jaccard term alone of the N items against themselves, as fp16 rows
//                           (reidmi_rr_jaccard_self_rows) or as the count / union / border passes
//                           of DBSCAN on it (reidmi_dbscan_jaccard; the O(N) kernels: cluster.h)
// Boundary: from V_qe and its inverted index to final distances, rank lists or cluster labels.  JCH
// (rerank.h) is read only here: the kernels' chunk and every grid and byte count derived from it,
// which is why the DBSCAN passes over the chunks live here and not in cluster.hip.
#include "backend.h"
#include "cluster.h"
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
// reranking.py:93: jaccard_jac_bits, the distance the self form stops at), the blend in fp32
// (reranking.py:95).  The one definition for every Jaccard kernel, matrix, selecting or self form.
__device__ __forceinline__ uint16_t jaccard_jac_bits(uint16_t tm) {
    const float tv = h2f_bits(tm);
    const uint16_t den = f2h_bits(2.0f - tv);
    const uint16_t qt = f2h_bits(tv / h2f_bits(den));
    return f2h_bits(1.0f - h2f_bits(qt));
}

__device__ __forceinline__ float jaccard_blend_one(uint16_t tm, float od, float dv, float lam, float lam_f) {
    const uint16_t jac = jaccard_jac_bits(tm);
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

// The walk of one (row i, chunk) over sorted lists, for every kernel that has tmin (fp16 bits, JCH
// entries in LDS, zeroed, a barrier passed): on return, behind its last barrier, tmin[r - base] is
// temp_min of chunk column r.  cbnd: the bounds of jaccard_bounds_kernel, nb1 = chunks + 1 per
// column; base: the first row index of the chunk.
__device__ __forceinline__ void jaccard_walk(uint16_t* tmin, const Rows& Vq, int64_t i, int64_t base,
                                             const int32_t* __restrict__ irow, const uint16_t* __restrict__ ival,
                                             const int64_t* __restrict__ cbnd, int64_t chunk, int nb1) {
    const int nz = Vq.len(i);
    const int64_t qb = Vq.beg(i);
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
            const int64_t p0 = cbnd[(int64_t)c * nb1 + chunk], p1 = cbnd[(int64_t)c * nb1 + chunk + 1];
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
    jaccard_walk(tmin, Vq, i, base, irow, ival, cbnd, blockIdx.x, (int)gridDim.x + 1);
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

// ----------------------------------------------------------- the self form
// jd(i, j) = the Jaccard term alone (reranking.py:86-93, jaccard_jac_bits) of every row i against
// every column j of the same N items: Q = 0 in the bounds, the same walk, so temp_min has the
// matrix form's bits.  One workgroup per (row, chunk), the chunks of a row adjacent in the grid.
//   JS_ROWS      the fp16 bits of the chunk's jd -> out (the dense form: small N, tests)
//   DBS_COUNT    hits of row i in the chunk (jd <= eps, or the diagonal): one atomic add
//   DBS_UNION    core rows only: every core hit j > i joins i's tree (cluster.h)
//   DBS_BORDER   non-core rows only: the smallest final parent[] among the core hits, one atomicMin
// jd < 1 only where V_qe[i] and V_qe[j] share a column, that is, where a list of one of V_qe[i]'s
// columns has an entry in the chunk: a workgroup that finds all its slices empty returns before it
// zeroes tmin (JS_ROWS: after writing jd = 1), and eps < 1 makes that exact.  The chunk that holds
// i itself is never skipped (the diagonal counts whatever V_qe[i] holds).  UNION and BORDER return
// at once for rows that are not of their kind.
constexpr int JS_ROWS = 3;  // beside DbsPass

template <int PASS>
__global__ __launch_bounds__(256) void jaccard_self_kernel(int64_t N, int64_t row0, int nch, Rows Vq,
                                                           const int32_t* __restrict__ irow,
                                                           const uint16_t* __restrict__ ival,
                                                           const int64_t* __restrict__ cbnd, float eps,
                                                           const uint8_t* __restrict__ core,
                                                           int32_t* __restrict__ counts, int32_t* parent,
                                                           int32_t* __restrict__ border, uint16_t* __restrict__ out,
                                                           int64_t ldo) {
    __shared__ uint16_t tmin[JCH];
    __shared__ int s_acc;  // COUNT: the chunk's hits; BORDER: its smallest root
    const int64_t y = blockIdx.x / (unsigned)nch;
    const int64_t chunk = blockIdx.x - y * nch;
    const int64_t i = row0 + y;
    if constexpr (PASS == DBS_UNION || PASS == DBS_BORDER) {
        if ((core[i] != 0) != (PASS == DBS_UNION)) return;
    }
    const int64_t base = chunk * JCH;
    const int64_t end = base + JCH < N ? base + JCH : N;
    const int span = (int)(end - base);
    const int nz = Vq.len(i);
    const int64_t qb = Vq.beg(i);
    bool any = base <= i && i < end;
    for (int e = threadIdx.x; e < nz && !any; e += blockDim.x) {
        const int64_t b = (int64_t)Vq.col[qb + e] * (nch + 1) + chunk;
        any = cbnd[b + 1] > cbnd[b];
    }
    if (!__syncthreads_or(any)) {
        if constexpr (PASS == JS_ROWS) {
            const uint16_t one = jaccard_jac_bits(0);
            for (int t = threadIdx.x; t < span; t += blockDim.x) out[y * ldo + base + t] = one;
        }
        return;
    }
    for (int t = threadIdx.x; t < span; t += blockDim.x) tmin[t] = 0;
    if (threadIdx.x == 0) s_acc = PASS == DBS_BORDER ? DBS_NONE : 0;
    __syncthreads();
    jaccard_walk(tmin, Vq, i, base, irow, ival, cbnd, chunk, nch + 1);
    if constexpr (PASS == JS_ROWS) {
        for (int t = threadIdx.x; t < span; t += blockDim.x) out[y * ldo + base + t] = jaccard_jac_bits(tmin[t]);
    } else {
        int acc = PASS == DBS_BORDER ? DBS_NONE : 0;
        for (int t = threadIdx.x; t < span; t += blockDim.x) {
            const int64_t j = base + t;
            const bool hit = h2f_bits(jaccard_jac_bits(tmin[t])) <= eps;
            if constexpr (PASS == DBS_COUNT) {
                acc += hit || j == i;
            } else if constexpr (PASS == DBS_UNION) {
                if (hit && i < j && core[j] != 0) dbs_union(parent, (int)i, (int)j);
            } else {
                if (hit && core[j] != 0) {
                    const int r = parent[j];  // final roots
                    acc = r < acc ? r : acc;
                }
            }
        }
        if constexpr (PASS == DBS_COUNT) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if ((threadIdx.x & 63) == 0 && acc != 0) atomicAdd(&s_acc, acc);
            __syncthreads();
            if (threadIdx.x == 0 && s_acc != 0) atomicAdd(&counts[i], s_acc);
        } else if constexpr (PASS == DBS_BORDER) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int u = __shfl_xor(acc, o, 64);
                acc = u < acc ? u : acc;
            }
            if ((threadIdx.x & 63) == 0 && acc != DBS_NONE) atomicMin(&s_acc, acc);
            __syncthreads();
            if (threadIdx.x == 0 && s_acc != DBS_NONE) atomicMin(&border[i], s_acc);
        }
    }
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

// The self form's launches.  A launch holds fewer than 2^31 threads: the bounds go column slab by
// column slab (a slab's lists are addressed through the same irow, its bounds behind the previous
// slab's), a pass row slab by row slab.
constexpr int64_t JS_THREADS = 1ll << 31;

static int jaccard_self_bounds(int64_t N, const int64_t* coff, const int32_t* irow, int64_t* cbnd, hipStream_t s) {
    const int nch = ceil_div(N, JCH);
    const int64_t per = JS_THREADS / (nch + 1);
    for (int64_t c0 = 0; c0 < N; c0 += per) {
        const int64_t n = N - c0 < per ? N - c0 : per;
        hipLaunchKernelGGL(jaccard_bounds_kernel, dim3(ceil_div(n * (nch + 1), 256)), dim3(256), 0, s, coff + c0, irow,
                           n, (int64_t)0, nch, cbnd + c0 * (nch + 1));
        RM_LAUNCHED();
    }
    return OK;
}

template <int PASS>
static int jaccard_self_run(int64_t N, int64_t lo, int64_t hi, const Rows& Vq, const int32_t* irow,
                            const uint16_t* ival, const int64_t* cbnd, float eps, const uint8_t* core,
                            int32_t* counts, int32_t* parent, int32_t* border, uint16_t* out, int64_t ldo,
                            hipStream_t s) {
    const int nch = ceil_div(N, JCH);
    const int64_t per = JS_THREADS / 256 / nch;  // >= 32: nch <= 2^18
    for (int64_t a = lo; a < hi; a += per) {
        const int64_t nb = hi - a < per ? hi - a : per;
        hipLaunchKernelGGL(jaccard_self_kernel<PASS>, dim3((unsigned)(nb * nch)), dim3(256), 0, s, N, a, nch, Vq, irow,
                           ival, cbnd, eps, core, counts, parent, border, out ? out + (a - lo) * ldo : nullptr, ldo);
        RM_LAUNCHED();
    }
    return OK;
}

// workspace of reidmi_dbscan_jaccard: the O(N) state (cluster.h) | the chunk bounds
static bool dbs_jaccard_ws(int64_t N, DbsState* w, int64_t* bytes) {
    if (!dbs_state(N, w)) return false;
    *bytes = w->bytes + jaccard_bounds_bytes(N, N);
    return true;
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

REIDMI_API int reidmi_rr_jaccard_self_rows(int64_t N, int64_t lo, int64_t hi, const int64_t* qoff, const int32_t* qcol,
                                           const uint16_t* qval, const int64_t* coff, const int32_t* irow,
                                           const uint16_t* ival, uint16_t* out, int64_t ldo, void* bounds,
                                           int64_t bounds_bytes, void* stream) {
    RM_REQUIRE(N >= 1 && N < (1ll << 31) && 0 <= lo && lo <= hi && hi <= N && ldo >= N,
               "rr_jaccard_self_rows: bad shape or row range (need 1 <= N < 2^31, 0 <= lo <= hi <= N, ldo >= N)");
    RM_REQUIRE(qoff && qcol && qval && coff && irow && ival && out, "rr_jaccard_self_rows: inputs and out required");
    RM_REQUIRE(bounds && ((uintptr_t)bounds & 7) == 0 && bounds_bytes >= jaccard_bounds_bytes(N, N),
               "rr_jaccard_self_rows: bounds of reidmi_rr_jaccard_bounds_bytes(N, N) bytes (8-byte aligned) required");
    if (hi == lo) return OK;
    hipStream_t s = (hipStream_t)stream;
    int64_t* cbnd = (int64_t*)bounds;
    int rc;
    if ((rc = jaccard_self_bounds(N, coff, irow, cbnd, s))) return rc;
    return jaccard_self_run<JS_ROWS>(N, lo, hi, csr_rows(qoff, qcol, qval), irow, ival, cbnd, 0.0f, nullptr, nullptr,
                                     nullptr, nullptr, out, ldo, s);
}

REIDMI_API int64_t reidmi_dbscan_jaccard_workspace_bytes(int64_t N) {
    DbsState w;
    int64_t bytes;
    return dbs_jaccard_ws(N, &w, &bytes) ? bytes : -1;
}

// The passes of cluster.hip with the distance replaced: count, init, union, compress, border,
// labels; eps in fp16, as jd is.
REIDMI_API int reidmi_dbscan_jaccard(int64_t N, const int64_t* qoff, const int32_t* qcol, const uint16_t* qval,
                                     const int64_t* coff, const int32_t* irow, const uint16_t* ival, float eps,
                                     int min_samples, int32_t* labels, int32_t* counts, uint8_t* core,
                                     int32_t* n_clusters, void* ws, int64_t ws_bytes, void* stream) {
    RM_REQUIRE(N >= 1 && N < (1ll << 31), "dbscan_jaccard: bad shape (need 1 <= N < 2^31)");
    RM_REQUIRE(eps >= 0.0f && eps <= 3.402823466e+38f, "dbscan_jaccard: eps must be finite and >= 0");
    const float eps16 = (float)(_Float16)eps;  // round to nearest even, as numpy's float16(eps)
    RM_REQUIRE(eps16 < 1.0f, "dbscan_jaccard: eps must round to less than 1 in fp16 (jd = 1: no shared column)");
    RM_REQUIRE(min_samples >= 1, "dbscan_jaccard: need min_samples >= 1");
    RM_REQUIRE(qoff && qcol && qval && coff && irow && ival, "dbscan_jaccard: V_qe rows and their inverted index required");
    RM_REQUIRE(labels != nullptr && counts != nullptr && core != nullptr && n_clusters != nullptr,
               "dbscan_jaccard: labels, counts, core and n_clusters required");
    DbsState w;
    int64_t bytes;
    RM_REQUIRE(dbs_jaccard_ws(N, &w, &bytes) && ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= bytes,
               "dbscan_jaccard: workspace (reidmi_dbscan_jaccard_workspace_bytes, 16-byte aligned) required");
    hipStream_t s = (hipStream_t)stream;
    int32_t* parent = (int32_t*)((char*)ws + w.parent_off);
    int32_t* border = (int32_t*)((char*)ws + w.border_off);
    int32_t* number = (int32_t*)((char*)ws + w.number_off);
    int32_t* bsum = (int32_t*)((char*)ws + w.bsum_off);
    int64_t* cbnd = (int64_t*)((char*)ws + w.bytes);
    const Rows Vq = csr_rows(qoff, qcol, qval);
    int rc;
    RM_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)N * 4, s));
    if ((rc = jaccard_self_bounds(N, coff, irow, cbnd, s))) return rc;
    if ((rc = jaccard_self_run<DBS_COUNT>(N, 0, N, Vq, irow, ival, cbnd, eps16, core, counts, parent, border, nullptr,
                                          0, s)))
        return rc;
    if ((rc = dbs_init_launch(counts, N, min_samples, core, parent, border, s))) return rc;
    if ((rc = jaccard_self_run<DBS_UNION>(N, 0, N, Vq, irow, ival, cbnd, eps16, core, counts, parent, border, nullptr,
                                          0, s)))
        return rc;
    if ((rc = dbs_compress_launch(parent, N, s))) return rc;
    if ((rc = jaccard_self_run<DBS_BORDER>(N, 0, N, Vq, irow, ival, cbnd, eps16, core, counts, parent, border, nullptr,
                                           0, s)))
        return rc;
    return dbs_labels_launch(core, parent, border, number, bsum, w.nb, N, n_clusters, labels, s);
}
