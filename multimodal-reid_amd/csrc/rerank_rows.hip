// rerank_rows.hip — R3-R5 of the k-reciprocal re-rank (stage map: rerank.hip): the sparse rows, on
// gfx950.
//
//   R3  k-reciprocal expansion + V row    kreciprocal_kernel (LDS) / kreciprocal_generic_kernel (slab)
//   R4  query expansion V_qe              qe_kernel (LDS) / qe_generic_kernel (slab, deferred rows)
//       ELL -> CSR                        rows_len / scan / rows_pack
//   R5  inverted index (CSC)              csc_count / scan / csc_fill (/ csc_sort)
// Boundary: from the rank rows to V, V_qe and their inverted index.  The numpy-exact arithmetic
// (np_expf, pairwise_f32) and the sorting network live here with their only users.  The one-call
// driver (rerank.hip) reaches the kernels through v_rows_launch, qe_rows_launch,
// qe_generic_launch and csc_build (rerank.h), the same launchers the staged entry points use.
#include "rerank.h"

namespace reidmi {

// numpy float32 exp (simd_exp_f32, AVX512F/AVX2): see oracle/reid_oracle.c orc_np_expf.
__device__ __forceinline__ float np_expf(float x) {
    if (x != x) return x;
    if (x > 88.72283935546875f) return __builtin_inff();
    if (x < -103.97208404541015625f) return 0.0f;
    const float quad = __builtin_rintf(x * 1.442695040888963407359924681001892137f);
    float r = __builtin_fmaf(quad, -6.93145752e-1f, x);
    r = __builtin_fmaf(quad, -1.42860677e-6f, r);
    float num = __builtin_fmaf(5.082762527590693718096e-04f, r, 6.757896990527504603057e-03f);
    num = __builtin_fmaf(num, r, 5.114512081637298353406e-02f);
    num = __builtin_fmaf(num, r, 2.473615434895520810817e-01f);
    num = __builtin_fmaf(num, r, 7.257664613233124478488e-01f);
    num = __builtin_fmaf(num, r, 9.999999999980870924916e-01f);
    float den = __builtin_fmaf(2.159509375685829852307e-02f, r, -2.742335390411667452936e-01f);
    den = __builtin_fmaf(den, r, 1.0f);
    return __builtin_ldexpf(num / den, (int)quad);
}

// numpy float32 pairwise sum of a[0..n) (PW_BLOCKSIZE 128, 8 accumulators), iterative.
__device__ float pairwise_f32(const float* a, int n) {
    struct F { int off, n, n2, stage; float left; };
    F st[32];
    int sp = 0;
    st[sp++] = F{0, n, 0, 0, 0.f};
    float ret = 0.f;
    while (sp > 0) {
        F& f = st[sp - 1];
        if (f.stage == 0) {
            if (f.n < 8) {
                float res = 0.f;
                for (int i = 0; i < f.n; i++) res += a[f.off + i];
                ret = res; sp--; continue;
            }
            if (f.n <= 128) {
                float r[8];
                for (int j = 0; j < 8; j++) r[j] = a[f.off + j];
                int i;
                for (i = 8; i < f.n - (f.n % 8); i += 8)
                    for (int j = 0; j < 8; j++) r[j] += a[f.off + i + j];
                float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                for (; i < f.n; i++) res += a[f.off + i];
                ret = res; sp--; continue;
            }
            int n2 = f.n / 2;
            n2 -= n2 % 8;
            f.n2 = n2;
            f.stage = 1;
            F c{f.off, n2, 0, 0, 0.f};
            st[sp++] = c;
        } else if (f.stage == 1) {
            f.left = ret;
            f.stage = 2;
            F c{f.off + f.n2, f.n - f.n2, 0, 0, 0.f};
            st[sp++] = c;
        } else {
            ret = f.left + ret;
            sp--;
        }
    }
    return ret;
}

// The sorting network of every stage: the workgroup sorts k[0..n) ascending (keys below
// 0x7fffffff) and, with PAYLOAD, moves v[t] along with k[t].  k and v hold sort_len(n)
// entries; the tail is padded here.  One barrier per pass, the first one after the padding, so
// the caller's own writes of k[0..n) need none of their own.  Every thread of the workgroup
// calls it.  Inlined, so that a caller's LDS arrays stay LDS accesses.
template <bool PAYLOAD>
__device__ __forceinline__ void bitonic_sort(int32_t* k, uint16_t* v, int n) {
    const int P = sort_len(n);
    for (int t = n + threadIdx.x; t < P; t += blockDim.x) k[t] = 0x7fffffff;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P; t += blockDim.x) {
                const int o = t ^ j;
                if (o > t) {
                    const bool up = (t & kk) == 0;
                    const int32_t x = k[t], y = k[o];
                    if ((x > y) == up) {
                        k[t] = y;
                        k[o] = x;
                        if (PAYLOAD) {
                            const uint16_t a = v[t];
                            v[t] = v[o];
                            v[o] = a;
                        }
                    }
                }
            }
            __syncthreads();
        }
}

// ---------------------------------------------------------------- R3: V rows
__device__ __forceinline__ bool row_has(const int32_t* R, int64_t ldr, int32_t row, int kk, int32_t v) {
    const int32_t* p = R + (int64_t)row * ldr;
    for (int b = 0; b < kk; b++)
        if (p[b] == v) return true;
    return false;
}

// v in R[row][0, kk): every load issued before any compare (no early exit: the loads of a
// scan are independent, so they share one memory round trip per unrolled group)
__device__ __forceinline__ bool row_has_all(const int32_t* R, int64_t ldr, int32_t row, int kk, int32_t v) {
    const int32_t* p = R + (int64_t)row * ldr;
    bool hit = false;
#pragma unroll 16
    for (int b = 0; b < kk; b++) hit |= p[b] == v;
    return hit;
}

// The end of a V row, from the expansion list lst[0..n) of item i to output row b
// (reranking.py:66-71): np.unique, w = exp(-od[i, lst]), V[i, lst] = w / sum(w) in fp16.
// lst holds sort_len(n) ints and w n floats (LDS or the slab; inlined for either); wsum is
// 4 ints of LDS.  Reached by all 256 threads; the row is complete when it returns.
__device__ __forceinline__ void kr_finish_row(const DistSrc& ds, float dv, int64_t i, int64_t b, int32_t* lst, float* w,
                                              int n, int* wsum, int32_t* __restrict__ vcol,
                                              uint16_t* __restrict__ vval, int32_t* __restrict__ vnnz, int64_t vcap,
                                              int32_t* __restrict__ flags) {
    __shared__ int s_nu;
    __shared__ float s_sum;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    bitonic_sort<false>(lst, nullptr, n);
    // np.unique: thread t owns a contiguous segment, counts its first occurrences, and writes
    // them at the exclusive prefix of the counts (into w's storage, then back)
    const int seg = (n + 255) >> 8, s0 = tid * seg, s1 = s0 + seg < n ? s0 + seg : n;
    int cnt = 0;
    for (int t = s0; t < s1; t++) cnt += (t == 0 || lst[t] != lst[t - 1]);
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int pos = incl - cnt;
    for (int q = 0; q < wv; q++) pos += wsum[q];
    int32_t* u = (int32_t*)w;
    for (int t = s0; t < s1; t++)
        if (t == 0 || lst[t] != lst[t - 1]) u[pos++] = lst[t];
    if (tid == 255) s_nu = pos;  // (the last segment ends the list)
    __syncthreads();
    const int nu = s_nu;
    for (int t = tid; t < nu; t += blockDim.x) lst[t] = u[t];
    __syncthreads();
    for (int t = tid; t < nu; t += blockDim.x) w[t] = np_expf(-(dist_at(ds, i, lst[t]) / dv));
    __syncthreads();
    if (tid == 0) s_sum = pairwise_f32(w, nu);
    __syncthreads();
    if (nu > vcap) {  // cannot happen: nu <= kf (kh1 + 1) = the width rr_caps gives
        if (tid == 0) { atomicOr(flags, RR_SCRATCH); vnnz[b] = 0; }
        return;
    }
    const float sum = s_sum;
    for (int t = tid; t < nu; t += blockDim.x) {
        vcol[b * vcap + t] = lst[t];
        vval[b * vcap + t] = f2h_bits(w[t] / sum);
    }
    if (tid == 0) vnnz[b] = nu;
}

// One 256-thread workgroup per row i = row0 + blockIdx.x of od (output row blockIdx.x).
// R: initial_rank [N][ldr] (stable argsort prefix), rowdiv[N] the od divisors.  kf <= 64,
// kh1 <= 32 (rr_caps kr_fast).  The membership scans are spread over the workgroup: one
// (candidate a, depth f) pair per thread for the expansion's half-depth sets (bit f of a
// per-candidate mask), instead of one thread walking a's 26 x 26 scans one load at a time.
__global__ __launch_bounds__(256) void kreciprocal_kernel(DistSrc ds, const float* __restrict__ rowdiv,
                                                          const int32_t* __restrict__ R, int64_t ldr, int64_t row0,
                                                          int kf, int kh1, int32_t* __restrict__ vcol,
                                                          uint16_t* __restrict__ vval, int32_t* __restrict__ vnnz,
                                                          int64_t vcap, int32_t* __restrict__ flags) {
    __shared__ int32_t kr[64];
    __shared__ int32_t cand[64][32];          // R[a][f] of the k-reciprocal items a
    __shared__ uint32_t mpass[64], minkr[64];  // bit f: a in R[R[a][f]][:kh1]; and R[a][f] in kr
    __shared__ int32_t lst[KR_LST];
    __shared__ float w[KR_LST];
    __shared__ int wsum[4];
    __shared__ int s_nk, s_n;
    const int64_t b = blockIdx.x;
    const int64_t i = row0 + b;
    const int tid = threadIdx.x;
    // k-reciprocal set of i at depth k1 (reranking.py:53-56), kept in forward order
    if (tid < 64) {
        const int f = tid;
        bool keep = false;
        int32_t c = -1;
        if (f < kf) {
            c = R[i * ldr + f];
            keep = row_has_all(R, ldr, c, kf, (int32_t)i);
        }
        const unsigned long long m = __ballot(keep);
        const int pos = __popcll(m & ((1ull << f) - 1ull));
        if (keep) kr[pos] = c;
        if (f == 0) s_nk = __popcll(m);
        mpass[f] = 0;
        minkr[f] = 0;
    }
    __syncthreads();
    const int nk = s_nk;
    for (int t = tid; t < nk; t += blockDim.x) lst[t] = kr[t];
    if (tid == 0) s_n = nk;
    // expansion (reranking.py:57-65): candidate a's half-depth reciprocal set
    // {c = R[a][f], f < kh1 : a in R[c][:kh1]} is appended when more than 2/3 of it lies in the
    // k-reciprocal set; order is irrelevant (np.unique sorts)
    for (int p = tid; p < nk * kh1; p += blockDim.x) {
        const int ai = p / kh1, f = p - ai * kh1;
        const int32_t a = kr[ai];
        const int32_t c = R[(int64_t)a * ldr + f];
        cand[ai][f] = c;
        if (row_has_all(R, ldr, c, kh1, a)) {
            bool in = false;
            for (int q = 0; q < nk; q++) in |= kr[q] == c;
            atomicOr(&mpass[ai], 1u << f);
            if (in) atomicOr(&minkr[ai], 1u << f);
        }
    }
    __syncthreads();
    if (tid < nk) {
        const uint32_t mp = mpass[tid];
        const int nc = __popc(mp), inter = __popc(minkr[tid]);
        if ((double)inter > 2.0 / 3.0 * (double)nc) {
            int q = atomicAdd(&s_n, nc);
            for (int f = 0; f < kh1; f++)
                if ((mp >> f) & 1u) lst[q++] = cand[tid][f];
        }
    }
    __syncthreads();
    kr_finish_row(ds, rowdiv[i], i, b, lst, w, s_n, wsum, vcol, vval, vnnz, vcap, flags);
}

// R3 for any k1: the same steps as kreciprocal_kernel with the lists on a per-workgroup slab
// of global scratch (KrSlab; a workgroup's slab is only touched by its own threads, ordered by
// its barriers).  Rows b = blockIdx.x, + gridDim.x, ... < nrows.
__global__ __launch_bounds__(256) void kreciprocal_generic_kernel(DistSrc ds, const float* __restrict__ rowdiv,
                                                                  const int32_t* __restrict__ R, int64_t ldr,
                                                                  int64_t row0, int64_t nrows, int kf, int kh1,
                                                                  KrSlab sl, char* __restrict__ slab,
                                                                  int32_t* __restrict__ vcol,
                                                                  uint16_t* __restrict__ vval,
                                                                  int32_t* __restrict__ vnnz, int64_t vcap,
                                                                  int32_t* __restrict__ flags) {
    __shared__ int wsum[4];
    __shared__ int s_nk, s_n;
    char* base = slab + (int64_t)blockIdx.x * sl.bytes;
    int32_t* kr = (int32_t*)(base + sl.kr);
    int32_t* krs = (int32_t*)(base + sl.krs);
    int32_t* ncnt = (int32_t*)(base + sl.ncnt);
    int32_t* acc = (int32_t*)(base + sl.acc);
    int32_t* cs = (int32_t*)(base + sl.cs);
    int32_t* lst = (int32_t*)(base + sl.lst);
    float* w = (float*)(base + sl.w);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int64_t b = blockIdx.x; b < nrows; b += gridDim.x) {
        const int64_t i = row0 + b;
        // k-reciprocal set of i at depth kf in forward order (reranking.py:53-56)
        if (tid == 0) s_nk = 0;
        __syncthreads();
        for (int f0 = 0; f0 < kf; f0 += 256) {
            const int f = f0 + tid;
            bool keep = false;
            int32_t c = -1;
            if (f < kf) {
                c = R[i * ldr + f];
                keep = row_has(R, ldr, c, kf, (int32_t)i);
            }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) wsum[wv] = __popcll(m);
            __syncthreads();
            int before = s_nk;
            for (int q = 0; q < wv; q++) before += wsum[q];
            if (keep) kr[before + __popcll(m & ((1ull << lane) - 1ull))] = c;
            __syncthreads();
            if (tid == 0) s_nk += wsum[0] + wsum[1] + wsum[2] + wsum[3];
            __syncthreads();
        }
        const int nk = s_nk;
        // a sorted copy for the intersection counts (np.intersect1d of unique sets)
        for (int t = tid; t < nk; t += blockDim.x) krs[t] = kr[t];
        bitonic_sort<false>(krs, nullptr, nk);
        // each candidate's half-depth reciprocal set and the 2/3 overlap rule (reranking.py:57-65)
        for (int t = tid; t < nk; t += blockDim.x) {
            const int32_t a = kr[t];
            int32_t* ct = cs + (int64_t)t * kh1;
            int nc = 0;
            for (int f = 0; f < kh1; f++) {
                const int32_t c = R[(int64_t)a * ldr + f];
                if (row_has(R, ldr, c, kh1, a)) ct[nc++] = c;
            }
            int inter = 0;
            for (int q = 0; q < nc; q++) {
                int lo = 0, hi = nk;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (krs[mid] < ct[q]) lo = mid + 1; else hi = mid;
                }
                inter += lo < nk && krs[lo] == ct[q];
            }
            ncnt[t] = nc;
            acc[t] = (double)inter > 2.0 / 3.0 * (double)nc;
        }
        if (tid == 0) s_n = nk;
        for (int t = tid; t < nk; t += blockDim.x) lst[t] = kr[t];
        __syncthreads();
        for (int t = tid; t < nk; t += blockDim.x)
            if (acc[t]) {
                const int nc = ncnt[t];
                const int bs = atomicAdd(&s_n, nc);
                for (int q = 0; q < nc; q++) lst[bs + q] = cs[(int64_t)t * kh1 + q];
            }
        __syncthreads();
        kr_finish_row(ds, rowdiv[i], i, b, lst, w, s_n, wsum, vcol, vval, vnnz, vcap, flags);
        __syncthreads();  // the slab and the shared counters are reused by the next row
    }
}

// R3 over rows [row0, row0 + n) into the ELL (vcol, vval, vnnz) of width caps.vcap.
int v_rows_launch(const DistSrc& ds, const float* rowdiv, const int32_t* R, int64_t ldr, int64_t row0,
                  int64_t n, const RrCaps& c, char* krslab, int32_t* vcol, uint16_t* vval, int32_t* vnnz,
                  int32_t* flags, hipStream_t s) {
    if (n == 0) return OK;
    if (c.kr_fast) {
        hipLaunchKernelGGL(kreciprocal_kernel, dim3((unsigned)n), dim3(256), 0, s, ds, rowdiv, R, ldr, row0, c.kf, c.kh1,
                           vcol, vval, vnnz, c.vcap, flags);
    } else {
        const KrSlab sl = kr_slab(c.kf, c.kh1);
        hipLaunchKernelGGL(kreciprocal_generic_kernel, dim3((unsigned)(n < GEN_WG ? n : GEN_WG)), dim3(256), 0, s, ds,
                           rowdiv, R, ldr, row0, n, c.kf, c.kh1, sl, krslab, vcol, vval, vnnz, c.vcap, flags);
    }
    RM_LAUNCHED();
    return OK;
}

// --------------------------------------------------------------------- R4: QE
// V_qe[i] = fp16( (sum_{j<k2, in order} fp32(V[R[i][j]])) / k2 ) over the union of columns.
// Both kernels stage the k2 (column-sorted) rows back to back (row j at soff[j], soff[k2]
// entries in all), let the first occurrence of each column own it, and sort the owners'
// (column, bits) pairs by column.  The arrays are LDS in qe_kernel and a slab in
// qe_generic_kernel; the two steps below are inlined for either.

// Copies the k2 rows to scol / sval at soff[]; row_beg(j) = where row j starts in V.  Ends with
// a barrier.
template <typename RowBeg>
__device__ __forceinline__ void qe_stage_rows(const Rows& V, int k2, const int32_t* soff, int32_t* scol,
                                              uint16_t* sval, RowBeg row_beg) {
    for (int j = 0; j < k2; j++) {
        const int64_t rb = row_beg(j);
        const int n = soff[j + 1] - soff[j];
        for (int t = threadIdx.x; t < n; t += blockDim.x) {
            scol[soff[j] + t] = V.col[rb + t];
            sval[soff[j] + t] = V.val[rb + t];
        }
    }
    __syncthreads();
}

// Staged entry e of row j looks its column c up in the k2 rows in j order (binary search): if
// a row before j holds c, that one owns it; otherwise e sums c over the rows, divides by k2,
// rounds to fp16 and, unless that is zero, appends (c, bits) to ocol / oval while there are
// fewer than cap.  *s_no (LDS) is 0 on entry.  Returns the entry count, which runs on past cap
// (the caller's sign of an overflow).  Ends with a barrier.
__device__ __forceinline__ int qe_owner_sums(int k2, const int32_t* soff, const int32_t* scol, const uint16_t* sval,
                                             int32_t* ocol, uint16_t* oval, int cap, int* s_no) {
    const int tot = soff[k2];
    const float fk2 = (float)k2;
    for (int e = threadIdx.x; e < tot; e += blockDim.x) {
        int j = 0, hj = k2;  // the row of entry e: the largest j with soff[j] <= e
        while (j < hj) {
            const int mid = (j + hj + 1) >> 1;
            if (soff[mid] <= e) j = mid; else hj = mid - 1;
        }
        const int32_t c = scol[e];
        bool first = true;
        float acc = 0.f;
        for (int jj = 0; jj < k2; jj++) {
            int lo = soff[jj], hi = soff[jj + 1];
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (scol[mid] < c) lo = mid + 1; else hi = mid;
            }
            const bool hit = lo < soff[jj + 1] && scol[lo] == c;
            if (hit && jj < j) { first = false; break; }
            if (hit) acc += h2f_bits(sval[lo]);
        }
        if (!first) continue;
        const uint16_t h = f2h_bits(acc / fk2);
        if (h & 0x7fff) {
            const int p = atomicAdd(s_no, 1);
            if (p < cap) { ocol[p] = c; oval[p] = h; }
        }
    }
    __syncthreads();
    return *s_no;
}

// Row i = row0 + blockIdx.x (output row blockIdx.x), k2 <= QE_FAST_K2, everything in LDS.  A
// row whose k2 rows stage more than LCAP entries, or that produces more than QCAP, is appended
// to the deferred list (dlist[atomicAdd(dcount)] = b, qnnz[b] = 0) for qe_generic_kernel.
__global__ __launch_bounds__(256) void qe_kernel(const int32_t* __restrict__ R, int64_t ldr, int k2, int64_t row0,
                                                 Rows V, int32_t* __restrict__ qcol, uint16_t* __restrict__ qval,
                                                 int32_t* __restrict__ qnnz, int64_t qcap,
                                                 int32_t* __restrict__ dlist, int32_t* __restrict__ dcount) {
    __shared__ int32_t scol[LCAP];
    __shared__ uint16_t sval[LCAP];
    __shared__ int soff[33];
    __shared__ int32_t ocol[QCAP];
    __shared__ uint16_t oval[QCAP];
    __shared__ int s_no, s_bad;
    __shared__ int64_t s_rb[32];
    __shared__ int s_len[32];
    const int64_t b = blockIdx.x;
    const int64_t i = row0 + b;
    const int tid = threadIdx.x;
    // the k2 rows' extents in parallel (one thread each), then their offsets
    if (tid < k2) {
        const int64_t r = R[i * ldr + tid];
        s_rb[tid] = V.beg(r);
        s_len[tid] = V.len(r);
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int j = 0; j < k2; j++) {
            soff[j] = o;
            o += s_len[j];
        }
        soff[k2] = o;
        s_no = 0;
        s_bad = o > LCAP;
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) { qnnz[b] = 0; dlist[atomicAdd(dcount, 1)] = (int32_t)b; }
        return;
    }
    qe_stage_rows(V, k2, soff, scol, sval, [&](int j) { return s_rb[j]; });
    const int no = qe_owner_sums(k2, soff, scol, sval, ocol, oval, QCAP, &s_no);
    if (no > QCAP) {
        if (tid == 0) { qnnz[b] = 0; dlist[atomicAdd(dcount, 1)] = (int32_t)b; }
        return;
    }
    bitonic_sort<true>(ocol, oval, no);
    for (int t = tid; t < no; t += blockDim.x) {
        qcol[b * qcap + t] = ocol[t];
        qval[b * qcap + t] = oval[t];
    }
    if (tid == 0) qnnz[b] = no;
}

// The same for the rows i = row0 + b of all deferred rows b = dlist[d], d < *dcount (or all rows
// b < nrows when dlist is null), any k2, on a per-workgroup slab (QeSlab, sized for k2 rows of the
// V bound).  mode 0: qnnz[b] = the row's entry count only; mode 1: the row to CSR at qoff[b] (qnnz
// untouched); mode 2: the row to ELL row b (width qcap) and qnnz[b].
__global__ __launch_bounds__(256) void qe_generic_kernel(const int32_t* __restrict__ R, int64_t ldr, int k2,
                                                         int64_t row0, Rows V, const int32_t* __restrict__ dlist,
                                                         const int32_t* __restrict__ dcount, int64_t nrows, int mode,
                                                         int32_t* __restrict__ qcol, uint16_t* __restrict__ qval,
                                                         int32_t* __restrict__ qnnz, int64_t qcap,
                                                         const int64_t* __restrict__ qoff, QeSlab sl,
                                                         char* __restrict__ slab, int64_t tcap,
                                                         int32_t* __restrict__ flags) {
    __shared__ int s_tot, s_no;
    char* base = slab + (int64_t)blockIdx.x * sl.bytes;
    int32_t* soff = (int32_t*)(base + sl.soff);
    int32_t* scol = (int32_t*)(base + sl.scol);
    uint16_t* sval = (uint16_t*)(base + sl.sval);
    int32_t* okey = (int32_t*)(base + sl.okey);
    uint16_t* oval = (uint16_t*)(base + sl.oval);
    const int tid = threadIdx.x;
    const int64_t nd = dcount ? (int64_t)*dcount : nrows;
    for (int64_t d = blockIdx.x; d < nd; d += gridDim.x) {
        const int64_t b = dlist ? dlist[d] : d;
        const int64_t i = row0 + b;
        if (tid == 0) {
            int64_t o = 0;
            for (int j = 0; j < k2; j++) {
                soff[j] = (int32_t)o;
                o += V.len(R[i * ldr + j]);
            }
            soff[k2] = (int32_t)(o < tcap ? o : tcap);
            s_tot = o > tcap ? -1 : (int)o;
            s_no = 0;
        }
        __syncthreads();
        if (s_tot < 0) {  // beyond the slab (not for tcap from rr_caps)
            if (tid == 0) {
                atomicOr(flags, RR_SCRATCH);
                if (mode != 1) qnnz[b] = 0;
            }
            __syncthreads();
            continue;
        }
        qe_stage_rows(V, k2, soff, scol, sval, [&](int j) { return V.beg(R[i * ldr + j]); });
        const int no = qe_owner_sums(k2, soff, scol, sval, okey, oval, 0x7fffffff, &s_no);
        if (mode != 0) {
            bitonic_sort<true>(okey, oval, no);
            const int64_t o = mode == 1 ? qoff[b] : b * qcap;
            for (int t = tid; t < no; t += blockDim.x) { qcol[o + t] = okey[t]; qval[o + t] = oval[t]; }
        }
        if (mode != 1 && tid == 0) qnnz[b] = no;
        __syncthreads();  // the slab and the shared counters are reused by the next row
    }
}

// dlist[t] = t for t < n, *dcount = n (every row deferred)
__global__ void iota_kernel(int32_t* __restrict__ dlist, int64_t n, int32_t* __restrict__ dcount) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) dlist[t] = (int32_t)t;
    if (t == 0) *dcount = (int32_t)n;
}

// R4 main pass (qe_kernel, k2 <= QE_FAST_K2) over rows [row0, row0 + n): *dcount is cleared first
int qe_rows_launch(const int32_t* R, int64_t ldr, int k2, int64_t row0, int64_t n, const Rows& V, int32_t* qcol,
                   uint16_t* qval, int32_t* qnnz, int64_t qcap, int32_t* dlist, int32_t* dcount, hipStream_t s) {
    RM_CHECK_HIP(hipMemsetAsync(dcount, 0, 4, s));
    if (n == 0) return OK;
    hipLaunchKernelGGL(qe_kernel, dim3((unsigned)n), dim3(256), 0, s, R, ldr, k2, row0, V, qcol, qval, qnnz, qcap, dlist,
                       dcount);
    RM_LAUNCHED();
    return OK;
}

// qe_generic_kernel on wgs workgroups, each with its slab of sl.bytes
int qe_generic_launch(const int32_t* R, int64_t ldr, int k2, int64_t row0, const Rows& V, const int32_t* dlist,
                      const int32_t* dcount, int64_t nrows, int wgs, int mode, int32_t* qcol, uint16_t* qval,
                      int32_t* qnnz, int64_t qcap, const int64_t* qoff, const QeSlab& sl, char* slab, int64_t tcap,
                      int32_t* flags, hipStream_t s) {
    hipLaunchKernelGGL(qe_generic_kernel, dim3((unsigned)wgs), dim3(256), 0, s, R, ldr, k2, row0, V, dlist, dcount, nrows,
                       mode, qcol, qval, qnnz, qcap, qoff, sl, slab, tcap, flags);
    RM_LAUNCHED();
    return OK;
}

// ---------------------------------------------------- ELL -> CSR, row lengths
__global__ void rows_len_kernel(Rows V, int64_t n, int32_t* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) out[r] = V.len(r);
}

// exclusive scan of cnt[0..N) into off[0..N] (single workgroup, 1024 threads)
__global__ __launch_bounds__(1024) void scan_kernel(const int32_t* __restrict__ cnt, int64_t N, int64_t* __restrict__ off) {
    __shared__ int64_t part[1024];
    const int64_t per = (N + 1023) / 1024;
    const int64_t lo = threadIdx.x * per < N ? threadIdx.x * per : N;
    const int64_t hi = lo + per < N ? lo + per : N;
    int64_t s = 0;
    for (int64_t k = lo; k < hi; k++) s += cnt[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int t = 0; t < 1024; t++) { const int64_t v = part[t]; part[t] = acc; acc += v; }
        off[N] = acc;
    }
    __syncthreads();
    int64_t acc = part[threadIdx.x];
    for (int64_t k = lo; k < hi; k++) { off[k] = acc; acc += cnt[k]; }
}

// copy rows of V into CSR storage at off[] (one workgroup per row)
__global__ void rows_pack_kernel(Rows V, const int64_t* __restrict__ off, int32_t* __restrict__ col,
                                 uint16_t* __restrict__ val) {
    const int64_t r = blockIdx.x;
    const int64_t s = V.beg(r), d = off[r];
    const int n = V.len(r);
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        col[d + t] = V.col[s + t];
        val[d + t] = V.val[s + t];
    }
}

// ------------------------------------------------------------------ R5: CSC
// invIndex[c] = rows r with V_qe[r, c] != 0 (reranking.py:80-82): per-column counts, an
// exclusive scan, an atomic fill, and (staged driver) a per-column sort by row.
__global__ void csc_count_kernel(Rows V, int64_t N, int32_t* __restrict__ cnt) {
    const int64_t r = blockIdx.x;
    const int64_t s = V.beg(r);
    const int n = V.len(r);
    for (int t = threadIdx.x; t < n; t += blockDim.x) atomicAdd(&cnt[V.col[s + t]], 1);
}

// Unsorted inverted index by atomic fill (the one-call paths: sizes unknown on the host).
__global__ void csc_fill_kernel(Rows V, int64_t N, const int64_t* __restrict__ off, int32_t* __restrict__ cur,
                                int32_t* __restrict__ irow, uint16_t* __restrict__ ival) {
    const int64_t r = blockIdx.x;
    const int64_t s = V.beg(r);
    const int n = V.len(r);
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        const int32_t c = V.col[s + t];
        const int64_t p = off[c] + atomicAdd(&cur[c], 1);
        irow[p] = (int32_t)r;
        ival[p] = V.val[s + t];
    }
}

// Sort each inverted list by row (reranking.py:80-82 lists rows ascending; the staged
// Jaccard kernel binary-searches a list for a chunk's row range).  One workgroup per column;
// rows are unique within a column, so any sort is the stable one.  Lists of up to
// CSC_LDS entries are bitonic-sorted in LDS; longer ones (hub items in very large galleries)
// in a power-of-two padded slice of a global scratch at 2 * off[c] (>= the padded length,
// since sort_len(len) < 2 len).
constexpr int CSC_LDS = 4096;

__global__ __launch_bounds__(256) void csc_sort_kernel(const int64_t* __restrict__ off, int32_t* __restrict__ irow,
                                                       uint16_t* __restrict__ ival, int32_t* __restrict__ sk,
                                                       uint16_t* __restrict__ sv) {
    __shared__ int32_t lk[CSC_LDS];
    __shared__ uint16_t lv[CSC_LDS];
    const int64_t c = blockIdx.x;
    const int64_t b = off[c];
    const int n = (int)(off[c + 1] - b);
    if (n < 2) return;
    const bool in_lds = sort_len(n) <= CSC_LDS;
    int32_t* K = in_lds ? lk : sk + 2 * b;
    uint16_t* V = in_lds ? lv : sv + 2 * b;
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        K[t] = irow[b + t];
        V[t] = ival[b + t];
    }
    bitonic_sort<true>(K, V, n);
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        irow[b + t] = K[t];
        ival[b + t] = V[t];
    }
}

// The unsorted inverted index of V's N rows: off[0..N] and the entries irow / ival; cnt and cur
// are N ints of scratch each.
int csc_build(const Rows& V, int64_t N, int32_t* cnt, int32_t* cur, int64_t* off, int32_t* irow,
              uint16_t* ival, hipStream_t s) {
    RM_CHECK_HIP(hipMemsetAsync(cnt, 0, N * 4, s));
    RM_CHECK_HIP(hipMemsetAsync(cur, 0, N * 4, s));
    hipLaunchKernelGGL(csc_count_kernel, dim3((unsigned)N), dim3(256), 0, s, V, N, cnt);
    RM_LAUNCHED();
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, cnt, N, off);
    RM_LAUNCHED();
    hipLaunchKernelGGL(csc_fill_kernel, dim3((unsigned)N), dim3(256), 0, s, V, N, (const int64_t*)off, cur, irow, ival);
    RM_LAUNCHED();
    return OK;
}

struct CscPlan {
    int64_t cnt, cur, sk, sv, total;
};
static CscPlan csc_plan(int64_t N, int64_t nnz) {
    CscPlan p{};
    int64_t o = 0;
    p.cnt = o; o = align_up(o + N * 4, 256);
    p.cur = o; o = align_up(o + N * 4, 256);
    p.sk = o; o = align_up(o + 2 * nnz * 4, 256);  // padded sort scratch of long lists
    p.sv = o; o = align_up(o + 2 * nnz * 2, 256);
    p.total = o;
    return p;
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_rr_caps(int64_t N, int k1, int k2, int64_t* vcap, int64_t* qcap, int64_t* v_ws_bytes,
                              int64_t* qe_ws_bytes) {
    RM_REQUIRE(N > 0 && k1 >= 1 && k2 >= 1 && vcap && qcap, "rr_caps: bad arguments");
    const RrCaps c = rr_caps(N, k1, k2);
    *vcap = c.vcap;
    *qcap = QCAP;
    if (v_ws_bytes) *v_ws_bytes = c.kr_fast ? 0 : GEN_WG * kr_slab(c.kf, c.kh1).bytes;
    if (qe_ws_bytes) *qe_ws_bytes = GEN_WG * qe_slab(c.k2e, c.tcap).bytes;
    return OK;
}

REIDMI_API int reidmi_rr_v_rows(const float* feat, int64_t N, int64_t D, int64_t ldf, const float* sqn,
                                const float* rowmax, const int32_t* rank, int K, int64_t lo, int64_t hi, int k1,
                                int32_t* vcol, uint16_t* vval, int32_t* vnnz, void* ws, int64_t ws_bytes,
                                int32_t* flags, void* stream) {
    RM_REQUIRE(N > 0 && D > 0 && ldf >= D && 0 <= lo && lo <= hi && hi <= N && flags, "rr_v_rows: bad arguments");
    RM_REQUIRE(k1 >= 1 && K >= (k1 + 1 < N ? k1 + 1 : N), "rr_v_rows: k1 >= 1, K >= min(k1 + 1, N)");
    const RrCaps c = rr_caps(N, k1, 1);
    RM_REQUIRE(c.kr_fast || (ws && ws_bytes >= GEN_WG * kr_slab(c.kf, c.kh1).bytes),
               "rr_v_rows: workspace of reidmi_rr_caps' v_ws_bytes required");
    const DistSrc ds{nullptr, 0, 0, feat, ldf, (int)D, sqn};
    return v_rows_launch(ds, rowmax, rank, K, lo, hi - lo, c, (char*)ws, vcol, vval, vnnz, flags, (hipStream_t)stream);
}

REIDMI_API int reidmi_rr_row_offsets(const int32_t* nnz, int64_t rows, int64_t* off, void* stream) {
    RM_REQUIRE(rows >= 0 && off, "rr_row_offsets: bad arguments");
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, nnz, rows, off);
    RM_LAUNCHED();
    return OK;
}

REIDMI_API int reidmi_rr_pack(const int32_t* ell_col, const uint16_t* ell_val, const int32_t* nnz, int64_t rows,
                              int64_t cap, const int64_t* off, int32_t* col, uint16_t* val, void* stream) {
    RM_REQUIRE(rows >= 0 && cap > 0, "rr_pack: bad arguments");
    if (rows == 0) return OK;
    hipLaunchKernelGGL(rows_pack_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                       ell_rows(nnz, cap, ell_col, ell_val), off, col, val);
    RM_LAUNCHED();
    return OK;
}

// R4 main pass: rows lo..hi of V_qe into the ELL (qcol, qval, qnnz) of width
// reidmi_rr_caps' qcap; rows it cannot assemble in LDS get qnnz = 0 and are listed in
// dlist[0 .. *dcount) (dcount: device int32, cleared by the call) for reidmi_rr_qe_deferred.
REIDMI_API int reidmi_rr_qe_rows(const int32_t* rank, int K, int k2, int64_t lo, int64_t hi, const int64_t* voff,
                                 const int32_t* vcol, const uint16_t* vval, int32_t* qcol, uint16_t* qval,
                                 int32_t* qnnz, int32_t* dlist, int32_t* dcount, void* stream) {
    RM_REQUIRE(0 <= lo && lo <= hi && voff && dlist && dcount, "rr_qe_rows: bad arguments");
    RM_REQUIRE(k2 >= 2 && k2 <= K, "rr_qe_rows: 2 <= k2 <= K (k2 = 1 means V_qe = V)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = hi - lo;
    if (k2 <= QE_FAST_K2)
        return qe_rows_launch(rank, (int64_t)K, k2, lo, n, csr_rows(voff, vcol, vval), qcol, qval, qnnz, (int64_t)QCAP,
                              dlist, dcount, s);
    // k2 beyond the LDS kernel: every row is deferred
    RM_CHECK_HIP(hipMemsetAsync(qnnz, 0, n * 4, s));
    hipLaunchKernelGGL(iota_kernel, dim3(ceil_div(n > 0 ? n : 1, 256)), dim3(256), 0, s, dlist, n, dcount);
    RM_LAUNCHED();
    return OK;
}

// R4 for the rows deferred by reidmi_rr_qe_rows (dlist[0 .. n_def), relative to lo), on the
// workspace slabs (reidmi_rr_caps' qe_ws_bytes for the same N, k1, k2): mode 0 writes their
// entry counts to qnnz[b]; mode 1 writes the rows to CSR at qoff[b] (qoff: offsets of rows lo..hi).
REIDMI_API int reidmi_rr_qe_deferred(const int32_t* rank, int K, int k1, int k2, int64_t lo, int64_t N,
                                     const int64_t* voff, const int32_t* vcol, const uint16_t* vval,
                                     const int32_t* dlist, int64_t n_def, int mode, const int64_t* qoff, int32_t* qcol,
                                     uint16_t* qval, int32_t* qnnz, void* ws, int64_t ws_bytes, int32_t* flags,
                                     void* stream) {
    RM_REQUIRE(lo >= 0 && N > 0 && k1 >= 1 && voff && n_def >= 0 && (mode == 0 || mode == 1) && flags,
               "rr_qe_deferred: bad arguments");
    RM_REQUIRE(k2 >= 2 && k2 <= K, "rr_qe_deferred: 2 <= k2 <= K");
    RM_REQUIRE(mode == 0 ? qnnz != nullptr : (qoff && qcol && qval), "rr_qe_deferred: outputs");
    if (n_def == 0) return OK;
    RM_REQUIRE(dlist && n_def < (1ll << 31), "rr_qe_deferred: dlist");
    const RrCaps c = rr_caps(N, k1, k2);
    const QeSlab sl = qe_slab(k2, c.tcap);
    RM_REQUIRE(ws && ws_bytes >= GEN_WG * sl.bytes, "rr_qe_deferred: workspace of reidmi_rr_caps' qe_ws_bytes required");
    return qe_generic_launch(rank, (int64_t)K, k2, lo, csr_rows(voff, vcol, vval), dlist, (const int32_t*)nullptr, n_def,
                             (int)(n_def < GEN_WG ? n_def : GEN_WG), mode, qcol, qval, qnnz, (int64_t)0, qoff, sl,
                             (char*)ws, c.tcap, flags, (hipStream_t)stream);
}

REIDMI_API int64_t reidmi_rr_csc_workspace_bytes(int64_t N, int64_t nnz) { return csc_plan(N, nnz).total; }

// R5 for the staged driver: count per column, exclusive scan, atomic fill, per-column sort
// by row — the CSC of V_qe with every list in ascending row order (reranking.py:80-82).
REIDMI_API int reidmi_rr_csc(int64_t N, const int64_t* qoff, const int32_t* qcol, const uint16_t* qval, int64_t nnz,
                             int64_t* coff, int32_t* irow, uint16_t* ival, void* ws_, int64_t ws_bytes, void* stream) {
    RM_REQUIRE(N > 0 && N < (1ll << 31) && nnz >= 0 && nnz < 0x7fffffff && qoff && coff, "rr_csc: bad arguments");
    const CscPlan P = csc_plan(N, nnz);
    RM_REQUIRE(ws_bytes >= P.total, "rr_csc: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)ws_;
    int rc;
    if ((rc = csc_build(csr_rows(qoff, qcol, qval), N, (int32_t*)(ws + P.cnt), (int32_t*)(ws + P.cur), coff, irow, ival,
                        s)))
        return rc;
    if (nnz == 0) return OK;
    hipLaunchKernelGGL(csc_sort_kernel, dim3((unsigned)N), dim3(256), 0, s, (const int64_t*)coff, irow, ival,
                       (int32_t*)(ws + P.sk), (uint16_t*)(ws + P.sv));
    RM_LAUNCHED();
    return OK;
}
