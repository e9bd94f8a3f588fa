// rerank.h — what more than one source of the k-reciprocal re-rank needs (internal, not part of
// the C ABI; the stage map is at the head of rerank.hip).  The sources and their boundaries:
//   rerank_rank.hip     R2: rank rows (exact and with the fp16 pre-filter), small row utilities
//   rerank_rows.hip     R3-R5: V rows, query expansion, ELL -> CSR, the inverted index
//   rerank_jaccard.hip  R6+R7: the Jaccard blend, as a matrix or as rank lists; the Jaccard term
//                       alone of the set against itself, as rows or as DBSCAN's passes (cluster.h)
//   rerank.hip          the one-call driver over all of them
// Here: the capacity constants and the plans derived from them, the sparse row views and the
// distance source that pass from stage to stage, and the host launchers one source calls in
// another.  No kernel; a device helper only with its type (Rows' accessors, dist_at of DistSrc).
// JCH is read by rerank_jaccard.hip alone and dist_at by rerank_rows.hip alone, so a variant
// build of that one source with RR_JCH / DA_UNROLL is whole.
#pragma once
#include "common.h"

namespace reidmi {

// No capacity limits (the reference has none, reranking.py:51-78): every bound below only
// picks the kernel.  A V row holds at most kf (kh1 + 1) entries (the k-reciprocal set plus one
// half-depth set per accepted candidate), so its ELL width is that bound (rr_caps); rows whose
// expansion list fits KR_LST run in LDS (kreciprocal_kernel, k1 <= 61), others on workspace
// scratch (kreciprocal_generic_kernel).  A V_qe row of k2 <= QE_FAST_K2 rows with at most LCAP
// staged entries and QCAP outputs is assembled in LDS (qe_kernel); any other row is deferred to
// qe_generic_kernel, whose scratch is sized for the worst case (k2 rows of the V bound).
constexpr int KR_LST = 2048;   // expansion list of kreciprocal_kernel (LDS)
constexpr int QCAP = 4096;     // V_qe entries qe_kernel assembles in LDS
constexpr int LCAP = 6144;     // staged entries of the k2 rows in qe_kernel
constexpr int QE_FAST_K2 = 32;
constexpr int GEN_WG = 256;    // workgroups of the generic kernels (one per CU), each with its slab
#ifndef RR_JCH
#define RR_JCH 8192
#endif
constexpr int JCH = RR_JCH;   // gallery columns per Jaccard workgroup (fp16 accumulators in LDS)

// flags: a generic kernel found a row beyond the scratch bound it was sized for (cannot happen
// for bounds from rr_caps; a caller passing smaller scratch gets this instead of a fault)
enum RrFlag : int { RR_SCRATCH = 8 };

// smallest power of two >= max(n, 2): the padded length of a bitonic sort of n keys (select.h's
// pow2_ceil starts at 1)
__host__ __device__ inline int sort_len(int64_t n) {
    int64_t p = 2;
    while (p < n) p <<= 1;
    return (int)p;
}
static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) & ~(a - 1); }

// kf = min(k1 + 1, N), kh1 = min(round(k1 / 2) + 1, N): the two depths of reranking.py:53,60
static inline void kr_depths(int k1, int64_t N, int& kf, int& kh1) {
    kf = (int)(k1 + 1 < N ? k1 + 1 : N);
    const int kh = (int)__builtin_nearbyint((double)k1 / 2.0);  // int(np.around(k1/2))
    kh1 = (int)(kh + 1 < N ? kh + 1 : N);
}

struct RrCaps {
    int kf, kh1, K, k2e;
    int64_t vcap;  // entries of a V row (ELL width)
    int64_t tcap;  // staged entries of a V_qe row: k2e V rows
    int64_t qcap;  // entries of a V_qe row (one-call ELL width)
    bool kr_fast;
};
static inline RrCaps rr_caps(int64_t N, int k1, int k2) {
    RrCaps c{};
    kr_depths(k1, N, c.kf, c.kh1);
    int64_t K = k1 + 1 > k2 ? k1 + 1 : k2;
    c.K = (int)(K < N ? K : N);
    c.k2e = k2 < c.K ? k2 : c.K;  // initial_rank[i, :k2] has min(k2, N) entries
    const int64_t vb = (int64_t)c.kf * (c.kh1 + 1);
    c.vcap = vb < N ? vb : N;
    c.tcap = (int64_t)c.k2e * c.vcap;
    c.qcap = c.tcap < N ? c.tcap : N;
    c.kr_fast = c.kf <= 64 && c.kh1 <= 32 && vb <= KR_LST;  // (kreciprocal_kernel's masks)
    return c;
}

// Per-workgroup scratch of kreciprocal_generic_kernel (byte offsets in one slab)
struct KrSlab {
    int64_t kr, krs, ncnt, acc, cs, lst, w, bytes;
};
static inline KrSlab kr_slab(int kf, int kh1) {
    KrSlab s{};
    const int64_t nb = (int64_t)kf * (kh1 + 1);
    int64_t o = 0;
    s.kr = o; o = align_up(o + (int64_t)kf * 4, 16);
    s.krs = o; o = align_up(o + (int64_t)sort_len(kf) * 4, 16);
    s.ncnt = o; o = align_up(o + (int64_t)kf * 4, 16);
    s.acc = o; o = align_up(o + (int64_t)kf * 4, 16);
    s.cs = o; o = align_up(o + (int64_t)kf * kh1 * 4, 16);
    s.lst = o; o = align_up(o + (int64_t)sort_len(nb) * 4, 16);
    s.w = o; o = align_up(o + nb * 4, 16);
    s.bytes = o;
    return s;
}
// ... and of qe_generic_kernel
struct QeSlab {
    int64_t soff, scol, sval, okey, oval, bytes;
};
static inline QeSlab qe_slab(int k2e, int64_t tcap) {
    QeSlab s{};
    const int64_t P = sort_len(tcap);
    int64_t o = 0;
    s.soff = o; o = align_up(o + (int64_t)(k2e + 1) * 4, 16);
    s.scol = o; o = align_up(o + tcap * 4, 16);
    s.sval = o; o = align_up(o + tcap * 2, 16);
    s.okey = o; o = align_up(o + P * 4, 16);
    s.oval = o; o = align_up(o + P * 2, 16);
    s.bytes = o;
    return s;
}

// ------------------------------------------------------------------ row views
// A set of sparse rows: CSR (off != nullptr: row r = [off[r], off[r+1])) or fixed-capacity
// ELL (off == nullptr: row r = [r*cap, r*cap + nnz[r])).  Columns ascending in every row.
struct Rows {
    const int64_t* off;
    const int32_t* nnz;
    int64_t cap;
    const int32_t* col;
    const uint16_t* val;
    __device__ __forceinline__ int64_t beg(int64_t r) const { return off ? off[r] : r * cap; }
    __device__ __forceinline__ int len(int64_t r) const { return (int)(off ? off[r + 1] - off[r] : nnz[r]); }
};
static inline Rows csr_rows(const int64_t* off, const int32_t* col, const uint16_t* val) {
    return Rows{off, nullptr, 0, col, val};
}
static inline Rows ell_rows(const int32_t* nnz, int64_t cap, const int32_t* col, const uint16_t* val) {
    return Rows{nullptr, nnz, cap, col, val};
}

// Where original_dist entries come from: a materialised matrix (od != nullptr: entry
// (i, c) = od[(i - row0) * ld + c]) or recomputed from the features with the distance
// kernel's exact arithmetic — an fmaf chain over k ascending, then fmaf(-2, dot, |i|^2 +
// |c|^2) (distance.hip distmat_f32_kernel; the fp32 MFMA accumulates in the same order).
#ifndef DA_UNROLL
#define DA_UNROLL 16
#endif
struct DistSrc {
    const float* od;
    int64_t ld, row0;
    const float* feat;
    int64_t ldf;
    int D;
    const float* sqn;
};

__device__ __forceinline__ float dist_at(const DistSrc& s, int64_t i, int64_t c) {
    if (s.od) return s.od[(i - s.row0) * s.ld + c];
    const float* a = s.feat + i * s.ldf;
    const float* b = s.feat + c * s.ldf;
    float acc = 0.0f;
    int k = 0;
    if ((s.ldf & 3) == 0) {
        // unrolled so that many row loads are in flight ahead of the (sequential) fma chain
#pragma unroll DA_UNROLL
        for (; k + 4 <= s.D; k += 4) {
            const float4 x = *(const float4*)(a + k), y = *(const float4*)(b + k);
            acc = __builtin_fmaf(x.x, y.x, acc);
            acc = __builtin_fmaf(x.y, y.y, acc);
            acc = __builtin_fmaf(x.z, y.z, acc);
            acc = __builtin_fmaf(x.w, y.w, acc);
        }
    }
    for (; k < s.D; k++) acc = __builtin_fmaf(a[k], b[k], acc);
    return __builtin_fmaf(-2.0f, acc, s.sqn[i] + s.sqn[c]);
}

// ------------------------------------------------------------------ launchers that cross files
// rerank_rank.hip
int rowmax_launch(const float* x, int64_t rows, int64_t cols, int64_t ldx, float* out, hipStream_t s);
int transpose_launch(const float* D, const float* add, int64_t N, float* T, hipStream_t s);

// rerank_rows.hip
int v_rows_launch(const DistSrc& ds, const float* rowdiv, const int32_t* R, int64_t ldr, int64_t row0, int64_t n,
                  const RrCaps& c, char* krslab, int32_t* vcol, uint16_t* vval, int32_t* vnnz, int32_t* flags,
                  hipStream_t s);
int qe_rows_launch(const int32_t* R, int64_t ldr, int k2, int64_t row0, int64_t n, const Rows& V, int32_t* qcol,
                   uint16_t* qval, int32_t* qnnz, int64_t qcap, int32_t* dlist, int32_t* dcount, hipStream_t s);
int qe_generic_launch(const int32_t* R, int64_t ldr, int k2, int64_t row0, const Rows& V, const int32_t* dlist,
                      const int32_t* dcount, int64_t nrows, int wgs, int mode, int32_t* qcol, uint16_t* qval,
                      int32_t* qnnz, int64_t qcap, const int64_t* qoff, const QeSlab& sl, char* slab, int64_t tcap,
                      int32_t* flags, hipStream_t s);
int csc_build(const Rows& V, int64_t N, int32_t* cnt, int32_t* cur, int64_t* off, int32_t* irow, uint16_t* ival,
              hipStream_t s);

// rerank_jaccard.hip
int jaccard_scan_launch(const float* OD, int64_t ld, const float* rowdiv, int64_t Q, int64_t N, const Rows& Vq,
                        const int64_t* off, const int32_t* irow, const uint16_t* ival, uint16_t lam16, float lam_f,
                        float* out, int64_t ldo, hipStream_t s);

}  // namespace reidmi
