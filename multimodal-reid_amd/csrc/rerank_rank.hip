// rerank_rank.hip — R2 of the k-reciprocal re-rank (stage map: rerank.hip): the od divisors and
// initial_rank[:, :K] of row ranges (reranking.py:45-48), on gfx950.
//
//   exact form          distance rows in chunks (distance.hip) -> rowmax_kernel -> top-k (search.hip)
//   fp16 pre-filter     the fp16 MFMA product bounds every exact distance and only each row's
//                       candidates are recomputed: dense, sampled and triangle forms, all of them
//                       drivers of the GEMM's EPI_RRHI / EPI_RRSV epilogues (gemm_epilogue.h,
//                       gemm_rrsv.h) and prefilter.hip's selection kernels; the triangle form also in stages (reidmi_rr_tri_*,
//                       reidmi_rr_sv_*) for the sharded R2
//   row utilities       nonzero / gather_rows (the rows the pre-filter leaves for the exact form),
//                       the transpose of the one-call driver's non-symmetric input
// Boundary: everything up to the rank rows; nothing here reads a V row.  Other sources reach
// rowmax_kernel and transpose_kernel through rerank.h's launchers.
#include <algorithm>
#include "backend.h"
#include "gemm.h"
#include "prefilter.h"
#include "rerank.h"

namespace reidmi {

// ------------------------------------------------------------------ R2 helpers
__global__ void rowmax_kernel(const float* __restrict__ D, int64_t rows, int64_t cols, int64_t ld,
                              float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    float m = -__builtin_inff();
    for (int64_t j = lane; j < cols; j += 64) m = fmaxf(m, D[r * ld + j]);
    m = wave_max(m);
    if (lane == 0) out[r] = m;
}

int rowmax_launch(const float* x, int64_t rows, int64_t cols, int64_t ldx, float* out, hipStream_t s) {
    hipLaunchKernelGGL(rowmax_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, s, x, rows, cols, ldx, out);
    RM_LAUNCHED();
    return OK;
}

// T = (D + add)^T (a non-symmetric distance: od rows are D columns, reranking.py:46)
__global__ void transpose_kernel(const float* __restrict__ D, const float* __restrict__ add, int64_t N,
                                 float* __restrict__ T) {
    __shared__ float tile[32][33];
    const int64_t bx = (int64_t)blockIdx.x * 32, by = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 32 x 8
    for (int k = ty; k < 32; k += 8) {
        const int64_t r = by + k, c = bx + tx;
        if (r < N && c < N) tile[k][tx] = add ? D[r * N + c] + add[r * N + c] : D[r * N + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int64_t r = bx + k, c = by + tx;
        if (r < N && c < N) T[r * N + c] = tile[tx][k];
    }
}

int transpose_launch(const float* D, const float* add, int64_t N, float* T, hipStream_t s) {
    hipLaunchKernelGGL(transpose_kernel, dim3(ceil_div(N, 32), ceil_div(N, 32)), dim3(256), 0, s, D, add, N, T);
    RM_LAUNCHED();
    return OK;
}

// ------------------------------------------------- small row utilities (staged R2)
// Ordered compaction: idx[0 .. *count) = the positions p < n with flags[p] != 0, ascending
// (np.nonzero).  One 1024-thread workgroup: each pass ballots 1024 flags, the waves' counts
// are scanned in LDS.
__global__ __launch_bounds__(1024) void nonzero_kernel(const int32_t* __restrict__ flags, int64_t n,
                                                       int32_t* __restrict__ idx, int32_t* __restrict__ count) {
    __shared__ int wsum[16];
    __shared__ int s_base;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    for (int64_t p0 = 0; p0 < n; p0 += 1024) {
        const int64_t p = p0 + threadIdx.x;
        const bool k = p < n && flags[p] != 0;
        const uint64_t m = __ballot(k);
        if (lane == 0) wsum[wv] = __popcll(m);
        __syncthreads();
        int before = s_base;
        for (int w = 0; w < wv; w++) before += wsum[w];
        if (k) idx[before + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)p;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int w = 0; w < 16; w++) t += wsum[w];
            s_base += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = s_base;
}

// out[r][:] = x[row0 + idx[r]][:] (fp32 rows of d floats, 16-byte loads when aligned)
__global__ void gather_rows_kernel(const float* __restrict__ x, int64_t ldx, int64_t d, int64_t row0,
                                   const int32_t* __restrict__ idx, float* __restrict__ out, int64_t ldo) {
    const int64_t r = blockIdx.x;
    const float* src = x + (row0 + idx[r]) * ldx;
    float* dst = out + r * ldo;
    for (int64_t c = threadIdx.x; c < d; c += blockDim.x) dst[c] = src[c];
}

// ------------------------------------------------------------ the fp16 pre-filter's driver
// Sampled survivor form of the pre-filter (prefilter.hip rr_sample_kernel / rank_select_sv_kernel):
// the sample is every S-th item, ns = floor(N / S) rounded down to whole 256-column tiles; per
// row: the sample's bounds, then the survivor list (RR_SV_CAP pairs) instead of an N-wide row.
// The selection runs inside the GEMM's epilogue (gemm_rrsv.h rrsv_tile): survivors staged in LDS,
// row / column records by LDS-DMA, no global memory instruction per tile.  A first version
// appended straight to the rows' lists (an atomic round trip per row group and tile, its
// registers spilling the K-loop): 13.0 s at N = 1.01 M against 3.9 + 1.7 s for the dense form
// (profiles/r03/rerank_1m_in_epilogue.txt).  Staged in LDS: 3.7 s for all row passes; over
// the symmetric product's upper triangle (each pair tested for both its rows, one call):
// 1.98 s, the 1M re-rank 7.1 -> 4.3 s (profiles/r03/rerank_1m_triangle.txt).
constexpr int RR_SV_CAP_ = RR_SV_CAP;  // (prefilter.h, with RR_SAMPLE_STRIDE)

__global__ void rr_gather_norms_kernel(const float* __restrict__ sqn, const float* __restrict__ nrm, int64_t ns,
                                       int S, float* __restrict__ sqn_s, float* __restrict__ nrm_s) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ns) {
        sqn_s[t] = sqn[t * S];
        nrm_s[t] = nrm[t * S];
    }
}

// the survivor epilogue's column records (gemm_rrsv.h rrsv_tile) of the rectangular form: (squared
// norm, norm, -, -) of item c, zero past N
__global__ void rr_colrec_kernel(const float* __restrict__ sqn, const float* __restrict__ nrm, int64_t N, int64_t Np,
                                 float4* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < Np) out[t] = t < N ? make_float4(sqn[t], nrm[t], 0.f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The survivor GEMM's tile lists (gemm.h rr_tiles: M-tile << 16 | N-tile), bands of RR_BAND
// M-tiles walked N-major (the 32 tiles an XCD runs at once share 8 A and 4 W panels).
// Rectangular: tm x tn tiles.  Triangle (A = W, the whole symmetric product): the tiles with
// M-tile <= N-tile; band b (rows r0 = b B .. r0 + r - 1) holds, for N-tile nt >= r0,
// min(r, nt - r0 + 1) tiles.
constexpr int RR_BAND = 8;
__global__ void rr_rect_tiles_kernel(int tm, int tn, int* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)tm * tn) return;
    const int per = RR_BAND * tn, b = (int)(t / per), r = (int)(t - (int64_t)b * per);
    const int rows = tm - b * RR_BAND < RR_BAND ? tm - b * RR_BAND : RR_BAND;
    const int nt = r / rows, mt = b * RR_BAND + r - nt * rows;
    out[t] = mt << 16 | nt;
}

// prefilter.h's launchers of the three kernels above (the pre-filtered search shares them)
int rr_gather_norms_launch(const float* sqn, const float* nrm, int64_t ns, int S, float* sqn_s, float* nrm_s,
                           hipStream_t s) {
    hipLaunchKernelGGL(rr_gather_norms_kernel, dim3((unsigned)ceil_div(ns, 256)), dim3(256), 0, s, sqn, nrm, ns, S,
                       sqn_s, nrm_s);
    RM_LAUNCHED();
    return OK;
}

int rr_colrec_launch(const float* sqn, const float* nrm, int64_t N, int64_t Np, void* out, hipStream_t s) {
    hipLaunchKernelGGL(rr_colrec_kernel, dim3((unsigned)ceil_div(Np, 256)), dim3(256), 0, s, sqn, nrm, N, Np,
                       (float4*)out);
    RM_LAUNCHED();
    return OK;
}

int rr_rect_tiles_launch(int tm, int tn, int* out, hipStream_t s) {
    hipLaunchKernelGGL(rr_rect_tiles_kernel, dim3((unsigned)ceil_div((int64_t)tm * tn, 256)), dim3(256), 0, s, tm, tn,
                       out);
    RM_LAUNCHED();
    return OK;
}

__host__ __device__ inline int64_t rr_tri_band_count(int T, int b) {
    const int64_t r0 = (int64_t)b * RR_BAND, r = T - r0 < RR_BAND ? T - r0 : RR_BAND;
    return r * (r + 1) / 2 + (T - r0 - r) * r;
}

static int64_t rr_tri_tiles(int T) {
    int64_t n = 0;
    for (int b = 0; b * RR_BAND < T; b++) n += rr_tri_band_count(T, b);
    return n;
}

__global__ void rr_tri_tiles_kernel(int T, int* __restrict__ out) {
    const int b = blockIdx.x;
    __shared__ int64_t s_off;
    if (threadIdx.x == 0) {
        int64_t o = 0;
        for (int c = 0; c < b; c++) o += rr_tri_band_count(T, c);
        s_off = o;
    }
    __syncthreads();
    const int r0 = b * RR_BAND, r = T - r0 < RR_BAND ? T - r0 : RR_BAND;
    for (int nt = r0 + threadIdx.x; nt < T; nt += blockDim.x) {
        const int64_t k = nt - r0;
        const int64_t pos = s_off + (k < r ? k * (k + 1) / 2 : (int64_t)r * (r + 1) / 2 + (k - r) * r);
        const int c = k + 1 < r ? (int)k + 1 : r;
        for (int q = 0; q < c; q++) out[pos + q] = (r0 + q) << 16 | nt;
    }
}

// bytes of chunk the sampled form needs.  Rectangular (row passes): the column records, the
// sample's norms and the pass's tile list once, then per row the sample bounds, the survivor
// list, its counter, bound width and row record (the records padded to whole 256-row tiles:
// the epilogue's DMA reads them by tile).  Triangle (all rows in one call): the records of all
// items, the sample's norms, the tile list, the counters and widths, and the survivor lists of
// all rows (the sample bounds of a pass of rows overlay the lists before they are written).
static int64_t rr_sv_row_bytes(int64_t ns) { return 4 * ns + 8 * (int64_t)RR_SV_CAP_ + 4 + 4 + 16; }
// rows per pass of the rectangular form in a chunk of chunk_rows x Np floats (0: not applicable)
static int64_t rr_sv_pass_rows(int64_t N, int64_t Np, int64_t chunk_rows, int K, int S) {
    const int64_t ns = rr_sv_ns(N, S);
    if (ns < 256 || ns < 4 * K) return 0;
    // (the tile list of a pass of up to 65536 rows: 256 x Np / 256 ints = 4 Np bytes)
    const int64_t avail = chunk_rows * Np * 4 - 16 * Np - 8 * ns - 4 * Np - 256 * 16 - 256;
    int64_t r = avail / rr_sv_row_bytes(ns);
    r = r < 65536 ? r : 65536;
    return r >= 256 ? r / 256 * 256 : r >= 64 ? r : 0;  // whole 256-row tiles per pass when possible
}
// survivor capacity per row of the triangle form (0: not applicable: a list below 1024 pairs)
static int64_t rr_tri_cap(int64_t N, int64_t Np, int64_t chunk_rows, int K, int S) {
    const int64_t ns = rr_sv_ns(N, S);
    if (ns < 256 || ns < 4 * K || Np / 256 > 65536) return 0;
    const int64_t avail = chunk_rows * Np * 4 - 16 * Np - 8 * ns - 4 * rr_tri_tiles((int)(Np / 256)) - 8 * N - 1024;
    int64_t cap = avail / (8 * N) / 64 * 64;
    cap = cap < RR_SV_CAP_ ? cap : RR_SV_CAP_;
    return cap >= 1024 && 8 * N * cap >= 4 * ns * 256 ? cap : 0;
}

// ---- pieces of the triangle form, shared by rank_rows_f16 (one call over all rows) and the
// staged entry points reidmi_rr_tri_* (the sharded R2: the tile list split over ranks, the
// survivor lists of other ranks' rows exchanged, reranking.HipStages)
// sample norms (every S-th item), the upper-triangle tile list, the zero records past N
static int tri_init(const float* sqn, const float* nrm, int64_t N, int64_t Np, int64_t ns, int S, float4* meta,
                    float* sqn_s, float* nrm_s, int* tiles, hipStream_t s) {
    const int T = (int)(Np / 256);
    hipLaunchKernelGGL(rr_gather_norms_kernel, dim3((unsigned)ceil_div(ns, 256)), dim3(256), 0, s, sqn, nrm, ns, S,
                       sqn_s, nrm_s);
    RM_LAUNCHED();
    hipLaunchKernelGGL(rr_tri_tiles_kernel, dim3((unsigned)ceil_div(T, RR_BAND)), dim3(256), 0, s, T, tiles);
    RM_LAUNCHED();
    if (Np > N) RM_CHECK_HIP(hipMemsetAsync(meta + N, 0, (Np - N) * sizeof(float4), s));
    return OK;
}

// the sample's bounds of rows [a, a + nb) (EPI_RRHI against every S-th item) -> their records,
// widths and counters (rr_sample_kernel)
static int tri_sample(const _Float16* x16, int64_t Dp, const float* sqn, const float* nrm, const float* nmax2,
                      int64_t D, int K, int S, const float* sqn_s, const float* nrm_s, int64_t ns, int64_t a,
                      int64_t nb, float* hs, float4* meta, float* wrow, int32_t* cnt, int cap, hipStream_t s) {
    // the sample: W rows = every S-th item (row stride S * Dp)
    int r = rr_hi_sample_launch(x16 + a * Dp, Dp, x16, (int64_t)S * Dp, sqn, nrm, a, nb, sqn_s, nrm_s, ns, D, hs, s);
    return r ? r : rr_sample_launch(hs, ns, ns, sqn, nrm, nmax2, a, nb, K, (int)D, meta, wrow, cnt, cap, s);
}

int rr_hi_sample_launch(const void* a16, int64_t Dp, const void* w16, int64_t ldw, const float* rsqn,
                        const float* rnrm, int64_t row0, int64_t nb, const float* sqn_s, const float* nrm_s,
                        int64_t ns, int64_t D, float* hs, hipStream_t s) {
    EpiArgs es{};
    es.out = hs;
    es.ldc = ns;
    es.rr_sqn = rsqn;
    es.rr_nrm = rnrm;
    es.rr_csqn = sqn_s;
    es.rr_cnrm = nrm_s;
    es.rr_row0 = row0;
    es.rr_n = ns;
    rank_select_consts((int)D, es.rr_c);
    return gemm_f16(EPI_RRHI, a16, Dp, w16, ldw, nb, ns, Dp, es, s);
}

// the survivor GEMM (EPI_RRSV) over tiles [0, ntiles) of a tile list; tri: the list is (part
// of) the symmetric product's upper triangle and each pair above the diagonal is tested for both
// its rows
static int tri_survivors(const _Float16* x16, int64_t Dp, int64_t Np, const float* sqn, const float* nrm, int64_t N,
                         int64_t D, int64_t a, int64_t M, const float4* rowmeta, const float4* colrec, const int* tiles,
                         int64_t ntiles, bool tri, int32_t* cnt, int2* list, int cap, hipStream_t s) {
    // (the epilogue takes the items' norms from the records: sqn / nrm are not passed on)
    (void)sqn;
    (void)nrm;
    return rr_survivors_launch(x16 + a * Dp, x16, Dp, Np, N, D, M, rowmeta, colrec, tiles, ntiles, tri, cnt, list, cap,
                               s);
}

int rr_survivors_launch(const void* a16, const void* w16, int64_t Dp, int64_t Np, int64_t N, int64_t D, int64_t M,
                        const void* rowmeta, const void* colrec, const int* tiles, int64_t ntiles, bool tri,
                        int32_t* cnt, void* list, int cap, hipStream_t s) {
    if (ntiles <= 0) return OK;
    EpiArgs ev{};
    ev.rr_n = N;
    rank_select_consts((int)D, ev.rr_c);
    ev.rr_rowmeta = (const float4*)rowmeta;
    ev.rr_colrec = (const float4*)colrec;
    ev.rr_tiles = tiles;
    ev.rr_ntiles = ntiles;
    ev.rr_tri = tri;
    ev.sv_cnt = cnt;
    ev.sv_list = (int2*)list;
    ev.sv_cap = cap;
    GemmOpts persistent;
    persistent.tile = 2;  // the survivor epilogue's LDS buffers live in the 256 x 256 tile
    return gemm_f16(EPI_RRSV, a16, Dp, w16, Dp, M, Np, Dp, ev, s, persistent);
}

// rows per sample pass of the triangle form when its hs scratch overlays the N x cap lists
static int64_t tri_sample_rows(int64_t N, int64_t cap, int64_t ns) {
    return std::min<int64_t>(65536, 8 * N * cap / (4 * ns) / 256 * 256);
}

static int rank_rows_f16(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn, const float* nrm,
                         const float* nmax2, const void* feat16, int64_t Np, int64_t Dp, int64_t lo, int64_t hi,
                         int K, int32_t* rank_out, float* rowmax_out, int32_t* need, float* chunk,
                         int64_t chunk_rows, int S, hipStream_t s) {
    RM_REQUIRE(N > 0 && D > 0 && ldf >= D && 0 <= lo && lo <= hi && hi <= N && chunk_rows > 0 && K >= 1 && K <= N &&
                   K <= 64 && Np >= N && Np % 256 == 0 && Dp >= D && Dp % 64 == 0 && sqn && nrm && nmax2,
               "rr_rank_rows_f16: bad arguments");
    RM_REQUIRE(N < 0x7fffffff, "rr_rank_rows_f16: too many items");
    const _Float16* x16 = (const _Float16*)feat16;
    int rc;
    // (the survivor epilogue needs K >= 2 K-steps of the persistent tile: Dp >= 128)
    const bool sampled = Dp >= 128 && rr_sv_pass_rows(N, Np, chunk_rows, K, S) > 0;
    const int64_t tcap = sampled && lo == 0 && hi == N ? rr_tri_cap(N, Np, chunk_rows, K, S) : 0;
    const int T = (int)(Np / 256);
    auto sample = [&](float* hs, const float* sqn_s, const float* nrm_s, int64_t ns, int64_t a, int64_t nb,
                      float4* meta, float* wrow, int32_t* cnt, int cap) -> int {
        return tri_sample(x16, Dp, sqn, nrm, nmax2, D, K, S, sqn_s, nrm_s, ns, a, nb, hs, meta, wrow, cnt, cap, s);
    };
    auto survivors = [&](int64_t a, int64_t M, const float4* rowmeta, const float4* colrec, const int* tiles,
                         int64_t ntiles, bool tri, int32_t* cnt, int2* list, int cap) -> int {
        return tri_survivors(x16, Dp, Np, sqn, nrm, N, D, a, M, rowmeta, colrec, tiles, ntiles, tri, cnt, list, cap, s);
    };
    if (tcap > 0) {
        // triangle: every pair once (tiles with M-tile <= N-tile), tested for both its rows
        const int64_t ns = rr_sv_ns(N, S), ntri = rr_tri_tiles(T);
        float4* meta = (float4*)chunk;  // [Np]: row records = column records
        float* sqn_s = (float*)(meta + Np);
        float* nrm_s = sqn_s + ns;
        int* tiles = (int*)(nrm_s + ns);
        int32_t* cnt = (int32_t*)(tiles + ntri);
        float* wrow = (float*)(cnt + N);
        int2* list = (int2*)(((uintptr_t)(wrow + N) + 15) & ~(uintptr_t)15);  // [N][tcap]
        if ((rc = tri_init(sqn, nrm, N, Np, ns, S, meta, sqn_s, nrm_s, tiles, s))) return rc;
        const int64_t sp = tri_sample_rows(N, tcap, ns);  // rows per sample pass
        for (int64_t a = 0; a < N; a += sp) {
            const int64_t nb = N - a < sp ? N - a : sp;
            if ((rc = sample((float*)list, sqn_s, nrm_s, ns, a, nb, meta + a, wrow + a, cnt + a, (int)tcap))) return rc;
        }
        if ((rc = survivors(0, N, meta, meta, tiles, ntri, true, cnt, list, (int)tcap))) return rc;
        return rank_select_sv_launch(cnt, list, (int)tcap, wrow, feat, ldf, (int)D, sqn, 0, N, K, rank_out, rowmax_out,
                                     need, s);
    }
    if (sampled) {
        const int64_t pass = rr_sv_pass_rows(N, Np, chunk_rows, K, S);
        const int64_t ns = rr_sv_ns(N, S);
        float4* colrec = (float4*)chunk;  // [Np]
        float* sqn_s = (float*)(colrec + Np);
        float* nrm_s = sqn_s + ns;
        int* tiles = (int*)(nrm_s + ns);  // [pass / 256 (rounded up) x T]
        char* pbase = (char*)(((uintptr_t)(tiles + ceil_div(pass, 256) * (int64_t)T) + 15) & ~(uintptr_t)15);
        hipLaunchKernelGGL(rr_gather_norms_kernel, dim3((unsigned)ceil_div(ns, 256)), dim3(256), 0, s, sqn, nrm, ns, S,
                           sqn_s, nrm_s);
        RM_LAUNCHED();
        hipLaunchKernelGGL(rr_colrec_kernel, dim3((unsigned)ceil_div(Np, 256)), dim3(256), 0, s, sqn, nrm, N, Np,
                           colrec);
        RM_LAUNCHED();
        int tm_listed = -1;
        for (int64_t a = lo; a < hi; a += pass) {
            const int64_t nb = hi - a < pass ? hi - a : pass;
            float* hs = (float*)pbase;                                          // [nb][ns]
            int2* list = (int2*)(hs + nb * ns);                                 // [nb][cap]
            int32_t* cnt = (int32_t*)(list + nb * RR_SV_CAP_);                  // [nb]
            float* wrow = (float*)(cnt + nb);                                   // [nb]
            float4* meta = (float4*)(((uintptr_t)(wrow + nb) + 15) & ~(uintptr_t)15);  // [nb, padded to 256]
            const int tm = (int)ceil_div(nb, 256);
            if (tm != tm_listed) {
                hipLaunchKernelGGL(rr_rect_tiles_kernel, dim3((unsigned)ceil_div((int64_t)tm * T, 256)), dim3(256), 0, s,
                                   tm, T, tiles);
                RM_LAUNCHED();
                tm_listed = tm;
            }
            if ((rc = sample(hs, sqn_s, nrm_s, ns, a, nb, meta, wrow, cnt, RR_SV_CAP_))) return rc;
            if ((rc = survivors(a, nb, meta, colrec, tiles, (int64_t)tm * T, false, cnt, list, RR_SV_CAP_))) return rc;
            if ((rc = rank_select_sv_launch(cnt, list, RR_SV_CAP_, wrow, feat, ldf, (int)D, sqn, a, nb, K,
                                            rank_out + (a - lo) * K, rowmax_out + (a - lo), need + (a - lo), s)))
                return rc;
        }
        return OK;
    }
    for (int64_t a = lo; a < hi; a += chunk_rows) {
        const int64_t nb = hi - a < chunk_rows ? hi - a : chunk_rows;
        EpiArgs ea{};
        ea.out = chunk;
        ea.ldc = Np;
        ea.rr_sqn = sqn;
        ea.rr_nrm = nrm;
        ea.rr_row0 = a;
        ea.rr_n = N;
        rank_select_consts((int)D, ea.rr_c);
        if ((rc = gemm_f16(EPI_RRHI, x16 + a * Dp, Dp, x16, Dp, nb, Np, Dp, ea, s))) return rc;
        if ((rc = rank_select_launch(chunk, Np, feat, ldf, (int)D, sqn, nrm, nmax2, a, nb, N, K,
                                     rank_out + (a - lo) * K, rowmax_out + (a - lo), need + (a - lo), s)))
            return rc;
    }
    return OK;
}

// ---- The triangle form of R2 in stages (reranking.HipStages' sharded R2): every
// rank samples its own rows (records all-gathered), runs a contiguous share of the upper-triangle
// tile list over ALL rows (each pair tested for both its rows), sends the partial survivor lists
// of other ranks' rows to their owners (reidmi_rr_sv_pack -> all-to-all -> reidmi_rr_sv_merge)
// and selects its own rows: the union of the lists is the one-call triangle form's, and the
// selection sorts each list by (hi, index), so the rows come out with the same bits for any
// number of ranks, at the one-GPU triangle's total MFMA work.
__global__ void rr_sv_pack_kernel(const int32_t* __restrict__ cnt, const int2* __restrict__ list, int cap,
                                  int64_t rows, const int64_t* __restrict__ off, int2* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int n = cnt[r] < cap ? cnt[r] : cap;
    const int2* src = list + r * cap;
    int2* dst = out + off[r];
    for (int p = threadIdx.x & 63; p < n; p += 64) dst[p] = src[p];
}

__global__ void rr_sv_merge_kernel(int32_t* __restrict__ cnt, int2* __restrict__ list, int cap, int64_t rows,
                                   const int32_t* __restrict__ add_cnt, const int64_t* __restrict__ add_off,
                                   const int2* __restrict__ add) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int base = cnt[r], na = add_cnt[r];
    const int m = na < cap ? na : cap;  // entries the sender holds
    int2* dst = list + r * cap;
    const int2* src = add + add_off[r];
    for (int p = threadIdx.x & 63; p < m; p += 64)
        if ((int64_t)base + p < cap) dst[base + p] = src[p];
    __builtin_amdgcn_wave_barrier();
    if ((threadIdx.x & 63) == 0) {
        const int64_t t = (int64_t)base + na;
        cnt[r] = t < 0x3fffffff ? (int32_t)t : 0x3fffffff;  // > cap: the row overflows (need)
    }
}

}  // namespace reidmi

using namespace reidmi;

// Row maxima skipping NaN (fmaxf), the od divisors of reranking.py:46 for a block of
// distance rows (rowmax_kernel).
REIDMI_API int reidmi_rowmax_f32(const float* x, int64_t rows, int64_t cols, int64_t ldx, float* out, void* stream) {
    RM_REQUIRE(rows >= 0 && cols > 0 && ldx >= cols && out, "rowmax: bad arguments");
    if (rows == 0) return OK;
    return rowmax_launch(x, rows, cols, ldx, out, (hipStream_t)stream);
}

REIDMI_API int reidmi_nonzero_i32(const int32_t* flags, int64_t n, int32_t* idx, int32_t* count, void* stream) {
    RM_REQUIRE(n >= 0 && n < 0x7fffffff && count && (n == 0 || (flags && idx)), "nonzero: bad arguments");
    hipLaunchKernelGGL(nonzero_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, flags, n, idx, count);
    RM_LAUNCHED();
    return OK;
}

REIDMI_API int reidmi_gather_rows_f32(const float* x, int64_t ldx, int64_t d, int64_t row0, const int32_t* idx,
                                      int64_t n, float* out, int64_t ldo, void* stream) {
    RM_REQUIRE(n >= 0 && d > 0 && ldx >= d && ldo >= d && (n == 0 || (x && idx && out)), "gather_rows: bad arguments");
    if (n == 0) return OK;
    RM_REQUIRE(n < (1ll << 31), "gather_rows: too many rows");
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, x, ldx, d, row0, idx,
                       out, ldo);
    RM_LAUNCHED();
    return OK;
}

// ------------------------------------------------------------ staged re-ranking
// The same R1-R7 as row-range stages over caller-allocated, exactly sized buffers, so the
// N x N distance is never materialised (row chunks of it are) and the rows can be sharded
// over ranks with all-gathers between stages (multimodal_reid_amd/reranking.py).
REIDMI_API int reidmi_rr_rank_rows(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn, int64_t lo,
                                   int64_t hi, int K, int32_t* rank_out, float* rowmax_out, float* chunk,
                                   int64_t chunk_rows, void* stream) {
    RM_REQUIRE(N > 0 && D > 0 && ldf >= D && 0 <= lo && lo <= hi && hi <= N && chunk_rows > 0 && K >= 1 && K <= N,
               "rr_rank_rows: bad arguments");
    RM_REQUIRE(N < 0x7fffffff, "rr_rank_rows: too many items");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    for (int64_t a = lo; a < hi; a += chunk_rows) {
        const int64_t nb = hi - a < chunk_rows ? hi - a : chunk_rows;
        if ((rc = distmat_pre_launch(feat + a * ldf, nb, ldf, feat, N, ldf, D, sqn + a, sqn, chunk, N, s))) return rc;
        if ((rc = rowmax_launch(chunk, nb, N, N, rowmax_out + (a - lo), s))) return rc;
        if ((rc = topk_launch(chunk, nb, N, N, rowmax_out + (a - lo), K, rank_out + (a - lo) * K, nullptr, K, s)))
            return rc;
    }
    return OK;
}

// fp16 copy of the features for reidmi_rr_rank_rows_f16: [Np][Dp] (Np a multiple of 256 >= N,
// Dp a multiple of 64 >= D), zero-padded; *range_ok (device int32, set to 1 by the caller) is
// cleared when some |x| > 2^15 or is not finite (the pre-filter must not be used then).
REIDMI_API int reidmi_rr_feat16(const float* feat, int64_t N, int64_t D, int64_t ldf, void* feat16, int64_t Np,
                                int64_t Dp, int32_t* range_ok, void* stream) {
    RM_REQUIRE(Np % 256 == 0 && Dp % 64 == 0, "rr_feat16: Np % 256 == 0 and Dp % 64 == 0");
    return feat16_launch(feat, N, D, ldf, feat16, Np, Dp, range_ok, (hipStream_t)stream);
}

// Largest norm and squared norm over the items (out2[0], out2[1], device) for
// reidmi_rr_rank_rows_f16; once per feature set.
REIDMI_API int reidmi_rr_norm_max(const float* sqn, const float* nrm, int64_t N, float* out2, void* stream) {
    return norm_max_launch(sqn, nrm, N, out2, (hipStream_t)stream);
}

// reidmi_rr_rank_rows with an fp16 pre-filter: the fp16 MFMA product of the rows with the
// items bounds every exact distance, and only each row's candidates are recomputed with the
// exact chain.  Same rank_out / rowmax_out bits as reidmi_rr_rank_rows for the rows with
// need[r] = 0; rows with need[r] = 1 (concentrated or non-finite distances) are left for the
// exact rows.  nrm = sqrt(sqn) [N]; nmax2 = reidmi_rr_norm_max of sqn, nrm.  chunk: chunk_rows x
// Np fp32 of scratch.  Default: sample stride RR_SAMPLE_STRIDE (16), the selection inside the
// GEMM's epilogue (prefilter.hip, "R2 pre-filter with the selection in the GEMM"; the triangle
// form when one call covers all rows); below that size, or with reidmi_rr_rank_rows_f16_ex's
// stride 0 / 1, the GEMM writes the rows' bounds (chunk_rows x Np) and rank_select1 streams them.
// Same bits either way.
REIDMI_API int reidmi_rr_rank_rows_f16(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn,
                                       const float* nrm, const float* nmax2, const void* feat16, int64_t Np,
                                       int64_t Dp, int64_t lo, int64_t hi, int K, int32_t* rank_out,
                                       float* rowmax_out, int32_t* need, float* chunk, int64_t chunk_rows,
                                       void* stream) {
    return rank_rows_f16(feat, N, D, ldf, sqn, nrm, nmax2, feat16, Np, Dp, lo, hi, K, rank_out, rowmax_out, need,
                         chunk, chunk_rows, RR_SAMPLE_STRIDE, (hipStream_t)stream);
}

// The same with the sample stride chosen (tests: 0 = the dense form at any N).
REIDMI_API int reidmi_rr_rank_rows_f16_ex(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn,
                                          const float* nrm, const float* nmax2, const void* feat16, int64_t Np,
                                          int64_t Dp, int64_t lo, int64_t hi, int K, int32_t* rank_out,
                                          float* rowmax_out, int32_t* need, float* chunk, int64_t chunk_rows,
                                          int sample_stride, void* stream) {
    RM_REQUIRE(sample_stride >= 0, "rr_rank_rows_f16_ex: sample_stride >= 0");
    return rank_rows_f16(feat, N, D, ldf, sqn, nrm, nmax2, feat16, Np, Dp, lo, hi, K, rank_out, rowmax_out, need,
                         chunk, chunk_rows, sample_stride, (hipStream_t)stream);
}

// Rows one pass of reidmi_rr_rank_rows_f16(_ex) takes with a chunk of chunk_rows x Np floats:
// the sampled form's pass (> chunk_rows for large N), or chunk_rows for the dense form.
// sample_stride < 0: the stride reidmi_rr_rank_rows_f16 uses.
REIDMI_API int64_t reidmi_rr_rank_rows_f16_pass_rows(int64_t N, int64_t Np, int64_t chunk_rows, int K,
                                                     int sample_stride) {
    if (N <= 0 || Np < N || chunk_rows <= 0 || K < 1) return -1;
    const int S = sample_stride < 0 ? RR_SAMPLE_STRIDE : sample_stride;
    if (rr_tri_cap(N, Np, chunk_rows, K, S) > 0) return N;  // one call over all rows: the triangle form
    const int64_t p = rr_sv_pass_rows(N, Np, chunk_rows, K, S);
    return p > 0 ? p : chunk_rows;
}

// Triangle form's sizes for a chunk of chunk_rows x Np floats (the same as the one-call form
// picks, reidmi_rr_rank_rows_f16): *ntiles = tiles of the upper triangle, *cap = survivor slots
// per row (0: the triangle form does not apply), *ns = sample items, *sample_rows = rows per
// sample pass when its scratch (sample_rows x ns fp32) overlays the N x cap lists.
REIDMI_API int reidmi_rr_tri_plan(int64_t N, int64_t Np, int64_t chunk_rows, int K, int64_t* ntiles, int64_t* cap,
                                  int64_t* ns, int64_t* sample_rows) {
    RM_REQUIRE(N > 0 && Np >= N && Np % 256 == 0 && chunk_rows > 0 && K >= 1 && ntiles && cap && ns && sample_rows,
               "rr_tri_plan: bad arguments");
    const int S = RR_SAMPLE_STRIDE;
    *cap = K <= 64 ? rr_tri_cap(N, Np, chunk_rows, K, S) : 0;
    *ns = rr_sv_ns(N, S);
    *ntiles = Np / 256 <= 65536 ? rr_tri_tiles((int)(Np / 256)) : 0;
    *sample_rows = *cap > 0 ? tri_sample_rows(N, *cap, *ns) : 0;
    return OK;
}

// meta [Np] float4 (row / column records; the tail past N zeroed here), sqn_s / nrm_s [ns],
// tiles [ntiles] int32 (the upper-triangle tile list, band order)
REIDMI_API int reidmi_rr_tri_init(const float* sqn, const float* nrm, int64_t N, int64_t Np, int64_t ns, void* meta,
                                  float* sqn_s, float* nrm_s, int32_t* tiles, void* stream) {
    RM_REQUIRE(sqn && nrm && meta && sqn_s && nrm_s && tiles && N > 0 && Np >= N && Np % 256 == 0 && ns >= 256 &&
                   ns * RR_SAMPLE_STRIDE <= N,
               "rr_tri_init: bad arguments");
    return tri_init(sqn, nrm, N, Np, ns, RR_SAMPLE_STRIDE, (float4*)meta, sqn_s, nrm_s, tiles, (hipStream_t)stream);
}

// Records, widths and counters of rows [a, b) (meta / wrow / cnt indexed by item): the sample's
// bounds in passes of hs_rows rows through hs (hs_rows x ns fp32; may overlay the lists).
REIDMI_API int reidmi_rr_tri_sample(const void* feat16, int64_t Np, int64_t Dp, const float* sqn, const float* nrm,
                                    const float* nmax2, int64_t N, int64_t D, int K, const float* sqn_s,
                                    const float* nrm_s, int64_t ns, int64_t a, int64_t b, float* hs, int64_t hs_rows,
                                    void* meta, float* wrow, int32_t* cnt, int cap, void* stream) {
    RM_REQUIRE(feat16 && sqn && nrm && nmax2 && sqn_s && nrm_s && hs && meta && wrow && cnt && 0 <= a && a <= b &&
                   b <= N && Np >= N && Dp >= D && Dp % 64 == 0 && K >= 1 && K <= 64 && hs_rows > 0 && ns >= K &&
                   cap >= 1 && cap <= RR_SV_CAP_,
               "rr_tri_sample: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    for (int64_t x = a; x < b; x += hs_rows) {
        const int64_t nb = b - x < hs_rows ? b - x : hs_rows;
        if ((rc = tri_sample((const _Float16*)feat16, Dp, sqn, nrm, nmax2, D, K, RR_SAMPLE_STRIDE, sqn_s, nrm_s, ns, x, nb,
                             hs, (float4*)meta + x, wrow + x, cnt + x, cap, s)))
            return rc;
    }
    return OK;
}

// The survivor GEMM over tiles [t0, t1) of the triangle list, all N rows: appends to cnt [N] /
// list [N][cap] (cnt of rows not sampled on this rank must start at 0).
REIDMI_API int reidmi_rr_tri_survivors(const void* feat16, int64_t Np, int64_t Dp, const float* sqn, const float* nrm,
                                       int64_t N, int64_t D, const void* meta, const int32_t* tiles, int64_t t0,
                                       int64_t t1, int32_t* cnt, void* list, int cap, void* stream) {
    RM_REQUIRE(feat16 && sqn && nrm && meta && tiles && cnt && list && 0 <= t0 && t0 <= t1 && Np >= N && Np % 256 == 0 &&
                   Dp >= 128 && Dp % 64 == 0 && cap >= 1 && cap <= RR_SV_CAP_,
               "rr_tri_survivors: bad arguments");
    const float4* m = (const float4*)meta;
    return tri_survivors((const _Float16*)feat16, Dp, Np, sqn, nrm, N, D, 0, N, m, m, tiles + t0, t1 - t0, true, cnt,
                         (int2*)list, cap, (hipStream_t)stream);
}

// The selection of rows row0 .. row0 + rows from their lists (cnt / list / wrow indexed from
// row0): rank_out [rows][K], rowmax_out, need (rank_select_sv_kernel).
REIDMI_API int reidmi_rr_sv_select(const int32_t* cnt, const void* list, int cap, const float* wrow, const float* feat,
                                   int64_t ldf, int64_t D, const float* sqn, int64_t row0, int64_t rows, int K,
                                   int32_t* rank_out, float* rowmax_out, int32_t* need, void* stream) {
    RM_REQUIRE(cnt && list && wrow && feat && sqn && rank_out && rowmax_out && need && rows >= 0 && row0 >= 0,
               "rr_sv_select: bad arguments");
    return rank_select_sv_launch(cnt, (const int2*)list, cap, wrow, feat, ldf, (int)D, sqn, row0, rows, K, rank_out,
                                 rowmax_out, need, (hipStream_t)stream);
}

// The survivor lists of `rows` rows packed contiguously: out[off[r] + p] = list[r][p] for
// p < min(cnt[r], cap) (off = exclusive scan of those lengths).
REIDMI_API int reidmi_rr_sv_pack(const int32_t* cnt, const void* list, int cap, int64_t rows, const int64_t* off,
                                 void* out, void* stream) {
    RM_REQUIRE(cnt && list && off && rows >= 0 && cap >= 1 && (out || rows == 0), "rr_sv_pack: bad arguments");
    if (rows == 0) return OK;
    hipLaunchKernelGGL(rr_sv_pack_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, cnt,
                       (const int2*)list, cap, rows, off, (int2*)out);
    RM_LAUNCHED();
    return OK;
}

// Appends another rank's partial lists of the same rows: list[r][cnt[r] + p] = add[add_off[r] + p]
// while it fits cap; cnt[r] += add_cnt[r] (a total past cap marks the row's overflow, as the
// one-call form's counter does).
REIDMI_API int reidmi_rr_sv_merge(int32_t* cnt, void* list, int cap, int64_t rows, const int32_t* add_cnt,
                                  const int64_t* add_off, const void* add, void* stream) {
    RM_REQUIRE(cnt && list && add_cnt && add_off && rows >= 0 && cap >= 1, "rr_sv_merge: bad arguments");
    if (rows == 0) return OK;
    hipLaunchKernelGGL(rr_sv_merge_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, cnt,
                       (int2*)list, cap, rows, add_cnt, add_off, (const int2*)add);
    RM_LAUNCHED();
    return OK;
}
