// eval.hip — per-query CMC / AP of the CLIP-ReID eval path on gfx950.
//
//   reidmi_eval_rows       per-query CMC/AP of eval_func                evaluate.py:40-80
//   evf_finish_launch      the same ranks and AP from evalfeat.hip's histogram
//
// Bit-exact with numpy's float64 pairwise sums (the three summers below); the (value, index)
// order and the sort are select.h's.
#include "backend.h"
#include "common.h"
#include "select.h"

#include <algorithm>

namespace reidmi {

// ------------------------------------------------------------------- eval rows
// numpy pairwise sum (PW_BLOCKSIZE 128, 8 accumulators) of an n-long float64 vector that
// is zero except at sorted positions pos(0..m) with values val(t): adding +0.0 is exact,
// so only the tree structure over the nonzeros matters.  Iterative post-order walk.
// POS / VAL: callables t -> int64 position / double value.
template <typename POS, typename VAL>
__device__ double leaf_sum(POS pos, VAL val, int lo, int hi, int64_t off, int64_t n) {
    if (n < 8) {
        double res = 0.0;
        for (int t = lo; t < hi; t++) res += val(t);
        return res;
    }
    // r[] indexed only by constants (a run-time index would put it in scratch memory, one
    // memory round trip per access): each accumulator adds v or +0.0, and r + 0.0 == r for
    // every r reachable here (all accumulators start at +0.0 and the values are positive)
    double r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t main_end = n - (n % 8);
    int t = lo;
    for (; t < hi && pos(t) - off < main_end; t++) {
        const int p = (int)((pos(t) - off) & 7);
        const double v = val(t);
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] += p == k ? v : 0.0;
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; t < hi; t++) res += val(t);
    return res;
}

template <typename POS>
__device__ int lower_pos(POS pos, int lo, int hi, int64_t x) {
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (pos(mid) < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The walk's stack lives in LDS (`st`, PW_DEPTH frames, one walker lane): a private
// array indexed at run time would sit in scratch memory, one HBM round trip per access.
struct PwFrame {
    int64_t off, n, n2;
    int lo, hi, mid, stage;
    double left;
};
constexpr int PW_DEPTH = 48;

template <typename POS, typename VAL>
__device__ double pairwise_sparse(POS pos, VAL val, int m, int64_t n, PwFrame* st) {
    using Frame = PwFrame;
    int sp = 0;
    st[sp++] = Frame{0, n, 0, 0, m, 0, 0, 0.0};
    double ret = 0.0;
    while (sp > 0) {
        Frame& f = st[sp - 1];
        if (f.stage == 0) {
            if (f.lo == f.hi) { ret = 0.0; sp--; continue; }
            if (f.hi - f.lo == 1) { ret = val(f.lo); sp--; continue; }  // x + zeros == x in any order
            if (f.n <= 128) { ret = leaf_sum(pos, val, f.lo, f.hi, f.off, f.n); sp--; continue; }
            int64_t n2 = f.n / 2;
            n2 -= n2 % 8;
            f.n2 = n2;
            f.mid = lower_pos(pos, f.lo, f.hi, f.off + n2);
            f.stage = 1;
            Frame c{f.off, n2, 0, f.lo, f.mid, 0, 0, 0.0};
            st[sp++] = c;
        } else if (f.stage == 1) {
            f.left = ret;
            f.stage = 2;
            Frame c{f.off + f.n2, f.n - f.n2, 0, f.mid, f.hi, 0, 0, 0.0};
            st[sp++] = c;
        } else {
            ret = f.left + ret;
            sp--;
        }
    }
    return ret;
}

// The same sum as pairwise_sparse, for one wave: the m nonzeros' leaves of numpy's split tree
// (blocks of <= 128 elements; halving split rounded down to a multiple of 8) are found by
// the lanes in parallel (path bits + depth per nonzero), each leaf is summed by leaf_sum,
// and the leaves are combined in tree order by operator-precedence evaluation on the depth
// of each adjacent pair's lowest common split (the first differing path bit): O(m) serial
// steps instead of a walk over every split node.  Scratch (LDS, one wave): path[m], dep[m]
// ints, vals/ops stacks of AP_STACK entries.  Returns the sum on lane 0.
constexpr int AP_STACK = 34;

template <typename VAL>
__device__ double pairwise_tree_wave(const int* rk, VAL val, int m, int64_t n, uint32_t* path, int* dep,
                                     double* vals, int* ops) {
    const int lane = threadIdx.x & 63;
    for (int t = lane; t < m; t += 64) {
        int64_t off = 0, len = n;
        uint32_t pb = 0;
        int d = 0;
        while (len > 128) {
            int64_t n2 = len / 2;
            n2 -= n2 % 8;
            if ((int64_t)rk[t] - off < n2) len = n2;
            else { off += n2; len -= n2; pb |= 1u << d; }
            d++;
        }
        path[t] = pb;
        dep[t] = d;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    double res = 0.0;
    if (lane == 0) {
        int sp = 0, op = 0;
        int t = 0;
        while (t < m) {
            // leaf group [t, u): same path and depth
            int u = t + 1;
            while (u < m && path[u] == path[t] && dep[u] == dep[t]) u++;
            int64_t off = 0, len = n;
            for (int d = 0; d < dep[t]; d++) {  // the leaf's [off, off + len)
                int64_t n2 = len / 2;
                n2 -= n2 % 8;
                if ((path[t] >> d) & 1u) { off += n2; len -= n2; } else len = n2;
            }
            const double v = leaf_sum([&](int k) { return (int64_t)rk[k]; }, val, t, u, off, len);
            if (t > 0) {
                const int c = __builtin_ctz(path[t - 1] ^ path[t]);  // depth of the split between the leaves
                while (op > 0 && ops[op - 1] > c) {
                    const double b = vals[--sp];
                    vals[sp - 1] = vals[sp - 1] + b;
                    op--;
                }
                ops[op++] = c;
            }
            vals[sp++] = v;
            t = u;
        }
        while (op > 0) {
            const double b = vals[--sp];
            vals[sp - 1] = vals[sp - 1] + b;
            op--;
        }
        res = vals[0];
    }
    return res;
}

// pairwise_tree_wave's sum for m <= 64 with the leaves combined lane-parallel: lane t < m holds
// rk[t] (rk_l; rk is the same array in LDS, read for leaves holding several nonzeros).  Each
// leaf group's first lane sums its leaf (one nonzero: the value itself, x + zeros == x; more:
// leaf_sum over the group), then the splits are applied deepest first: at depth D every
// segment whose left boundary is a depth-D split adds itself into the segment on its left.
// Two depth-D boundaries never border the same segment (a shallower split lies between
// them), so this is pairwise_tree_wave's precedence evaluation step for step — the same
// additions, bit-identical — in (tree depth) wave steps instead of a serial chain over the
// leaves (that chain, even in registers, was ~27 % of a Market query:
// profiles/r02/eval_rows_phase_stamps.txt).
template <typename VAL>
__device__ double pairwise_tree_par(int rk_l, const int* rk, VAL val, int m, int64_t n) {
    const int lane = threadIdx.x & 63;
    const bool live = lane < m;
    uint32_t pb = 0;
    int d = 0;
    if (live) {
        int64_t off = 0, len = n;
        while (len > 128) {
            int64_t n2 = len / 2;
            n2 -= n2 % 8;
            if ((int64_t)rk_l - off < n2) len = n2;
            else { off += n2; len -= n2; pb |= 1u << d; }
            d++;
        }
    }
    const uint32_t ppb = (uint32_t)__shfl_up((int)pb, 1, 64);
    const int pd = __shfl_up(d, 1, 64);
    const bool head = live && (lane == 0 || ppb != pb || pd != d);
    const uint64_t heads = __ballot(head);
    double s = 0.0;
    int c = -1;  // depth of the split between the previous leaf and this one
    if (head) {
        const uint64_t above = (heads >> lane) >> 1;
        const int u = above ? lane + 1 + __builtin_ctzll(above) : m;
        if (u == lane + 1) {
            s = val(lane, rk_l);
        } else {
            int64_t off = 0, len = n;
            for (int e = 0; e < d; e++) {
                int64_t n2 = len / 2;
                n2 -= n2 % 8;
                if ((pb >> e) & 1u) { off += n2; len -= n2; } else len = n2;
            }
            s = leaf_sum([&](int k) { return (int64_t)rk[k]; }, [&](int k) { return val(k, rk[k]); }, lane, u, off,
                         len);
        }
        if (lane > 0) c = __builtin_ctz(ppb ^ pb);
    }
    int maxc = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(maxc, o, 64);
        maxc = t > maxc ? t : maxc;
    }
    uint64_t act = heads;
    for (int D = maxc; D >= 0; D--) {
        const bool on = (act >> lane) & 1;
        const uint64_t mrg = __ballot(on && c == D);
        if (!mrg) continue;
        const uint64_t nxt = lane < 63 ? act >> (lane + 1) : 0;
        const int R = nxt ? lane + 1 + __builtin_ctzll(nxt) : lane;
        const double sr = __shfl(s, R, 64);
        if (on && nxt && ((mrg >> R) & 1)) s = s + sr;
        act &= ~mrg;
    }
    return __shfl(s, 0, 64);
}

// Per query (evaluate.py:40-80): positives = gallery items with the query's pid and another
// camera, junk = same pid and same camera (removed, :55-56), everything else a kept
// negative.  With the positives sorted by (distance, index) — np.argsort(kind="stable") —
// the rank of positive k among the kept items is
//     rank_k = #{all j : key_j < key_pk} - #{junk i : key_i < key_pk},
// so one pass over the distance row that bins EVERY item by how many positives precede it
// (b(j) = #{p : key_p < key_j}; rank_k + 1 + junk_before(k) = sum_{t <= k} hist[t]) gives all
// ranks; AP = numpy's pairwise sum of (k+1)/(rank_k+1) at positions rank_k over the kept
// length, / m (:73-79); first = rank_0 (the CMC step, :65-68).
//
// Gallery labels packed once per eval_rows call: when the gallery pids span < 65535 values
// (every ReID benchmark), pid - min as uint16 (padded to a multiple of 8 with 0xFFFF), so
// each query's label pass reads 2 B per item instead of 8 (it is L2 traffic repeated by
// every query).  Otherwise the kernel reads the int64 pids.
struct EvLabels {
    int64_t lo, hi;  // min / max gallery pid, biased to unsigned order for the atomics
};

__device__ __forceinline__ uint64_t ord64(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
__device__ __forceinline__ int64_t unord64(uint64_t v) { return (int64_t)(v ^ 0x8000000000000000ull); }

__global__ void ev_minmax_init_kernel(unsigned long long* mm, int32_t* overflow) {
    mm[0] = ~0ull;
    mm[1] = 0ull;
    mm[2] = 0ull;  // eval_rows_kernel's arrival counter and huge-query count
    mm[3] = 0ull;  // "a query was deferred to eval_rows_kernel"
    *overflow = 0;
}

// min / max and the uint16 packing in ONE workgroup for galleries up to EV_PREP1_MAX (every
// ReID benchmark): one launch instead of three (each ~4-7 us at Market size, the kernel
// itself ~130 us).  Same outputs as ev_minmax_init/ev_minmax/ev_pack.
constexpr int64_t EV_PREP1_MAX = 1 << 18;

__global__ __launch_bounds__(1024) void ev_prep1_kernel(const int64_t* __restrict__ gp, int64_t G, int64_t G8,
                                                        unsigned long long* __restrict__ mm, uint16_t* __restrict__ pk,
                                                        int32_t* __restrict__ overflow) {
    __shared__ uint64_t slo[16], shi[16];
    const int tid = threadIdx.x;
    // 8 loads in flight per thread (a past-the-end item re-reads the last label: no effect on
    // min / max)
    constexpr int U = 8;
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t j0 = 0; j0 < G; j0 += 1024 * U) {
        int64_t v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 + u * 1024 + tid;
            v[u] = gp[j < G ? j : G - 1];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t o = ord64(v[u]);
            lo = o < lo ? o : lo;
            hi = o > hi ? o : hi;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t a = __shfl_xor(lo, off, 64), b = __shfl_xor(hi, off, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((tid & 63) == 0) { slo[tid >> 6] = lo; shi[tid >> 6] = hi; }
    __syncthreads();
    lo = slo[0];
    hi = shi[0];
    for (int w = 1; w < 16; w++) {
        lo = slo[w] < lo ? slo[w] : lo;
        hi = shi[w] > hi ? shi[w] : hi;
    }
    if (tid == 0) { mm[0] = lo; mm[1] = hi; mm[2] = 0ull; mm[3] = 0ull; *overflow = 0; }
    const int64_t plo = unord64(lo), phi = unord64(hi);
    if ((uint64_t)(phi - plo) >= 0xFFFFull) return;  // wide pid range: the int64 path
    for (int64_t j0 = 0; j0 < G8; j0 += 1024 * U) {
        int64_t v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 + u * 1024 + tid;
            v[u] = gp[j < G ? j : G - 1];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 + u * 1024 + tid;
            if (j < G8) pk[j] = j < G ? (uint16_t)(v[u] - plo) : (uint16_t)0xFFFF;
        }
    }
}

__global__ __launch_bounds__(256) void ev_minmax_kernel(const int64_t* __restrict__ gp, int64_t G,
                                                        unsigned long long* mm) {
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < G; j += (int64_t)gridDim.x * 256) {
        const uint64_t o = ord64(gp[j]);
        lo = o < lo ? o : lo;
        hi = o > hi ? o : hi;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t a = __shfl_xor(lo, off, 64), b = __shfl_xor(hi, off, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&mm[0], (unsigned long long)lo);
        atomicMax(&mm[1], (unsigned long long)hi);
    }
}

__global__ void ev_pack_kernel(const int64_t* __restrict__ gp, int64_t G, int64_t G8,
                               const unsigned long long* __restrict__ mm, uint16_t* __restrict__ pk) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G8) return;
    const int64_t lo = unord64(mm[0]), hi = unord64(mm[1]);
    if ((uint64_t)(hi - lo) >= 0xFFFFull) return;  // wide pid range: the int64 path
    pk[j] = j < G ? (uint16_t)(gp[j] - lo) : (uint16_t)0xFFFF;
}

// eval_rows_wg_kernel: one 256-thread workgroup (4 waves) per query, ~17 KiB of LDS, 8
// workgroups per CU.  Pass 1 streams the gallery labels (uint16-packed, L2-resident: every
// query reads the same lines) and compacts the indices of the query's pid (ballot + one LDS
// atomic per wave and hit); their cameras and distances then come in ONE round trip and
// split them into positives and junk; the positives are bitonic-sorted in LDS.  Pass 2 reads
// the distance row once (16-byte loads after a scalar head to 16-byte alignment), skipping
// items beyond the last positive, and bins the rest into an LDS histogram through a bucket
// table of the positives (no per-item binary search: that search was 2/3 of the kernel).
// Wave 0 scans the histogram into ranks and sums the AP lane-parallel.  Queries with more
// than EVW_MAXP positives or EVW_MAXJ junk items are left to eval_rows_kernel (valid = 2).
// Per-phase cycle stamps: profiles/r02/eval_rows_phase_stamps.txt.
constexpr int EVW_MAXP = 512, EVW_MAXJ = 256, EVW_T = 1024;

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void eval_rows_wg_kernel(
    const float* __restrict__ dist, int64_t G, int64_t ld, const int64_t* __restrict__ qp,
    const int64_t* __restrict__ gp, const int64_t* __restrict__ qc, const int64_t* __restrict__ gc,
    const unsigned long long* __restrict__ mm, const uint16_t* __restrict__ pk, int32_t* __restrict__ valid,
    int64_t* __restrict__ first, double* __restrict__ ap, int64_t* __restrict__ nkept, int32_t* __restrict__ large) {
    __shared__ float pv[EVW_MAXP];
    __shared__ int pi[EVW_MAXP];
    __shared__ int hist[EVW_MAXP + 1];
    __shared__ float jv[EVW_MAXJ];
    __shared__ int ji[EVW_MAXJ];
    __shared__ int s_m, s_nj, s_ns;
    __shared__ double tvals[AP_STACK];
    __shared__ int tops[AP_STACK];
    // bucket t: {bits of the first positive in it (+inf when none), S[t] | 1 << 16 when it holds
    // two or more}; entry T = {+inf, m} closes the table (S[T] = m)
    __shared__ int2 bucket[EVW_T + 1];
    __shared__ int trash[256];  // one histogram slot per thread for the items not binned
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t q = blockIdx.x;
    const float* row = dist + q * ld;
    const int64_t qpid = qp[q], qcam = qc[q];
    const uint64_t below = (1ull << lane) - 1;
    int* sidx = (int*)bucket;  // same-pid gallery indices of pass 1 (the bucket table comes later)
    constexpr int SCAP = EVW_MAXP + EVW_MAXJ;
    // the distance pass's layout (16-byte loads after a scalar head)
    const int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 2);  // scalar items before 16-B alignment
    const int h = head < G ? head : (int)G;
    const int nv = (int)((G - h) >> 2);  // float4 groups (G < 2^31)
    const float4* r4 = (const float4*)(row + h);
    constexpr int U2 = 4;
    float4 v[U2];
    auto load_chunk = [&](int g0) {  // past the row's end: reload its last group, not binned
#pragma unroll
        for (int u = 0; u < U2; u++) {
            const int g = g0 + u * 256 + tid;
            v[u] = r4[g < nv ? g : nv - 1];
        }
    };
    if (tid == 0) { s_m = 0; s_nj = 0; s_ns = 0; }
    __syncthreads();
    // ---- pass 1: labels -> indices of the gallery items with the query's pid (ballot
    // compaction, one LDS atomic per wave and hit).  Every workgroup reads the same label
    // lines, so each starts at its own chunk.
    auto take = [&](bool same, int64_t j) {
        const uint64_t ms = __ballot(same);
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_ns, __popcll(ms));
        base = __shfl(base, 0, 64);
        const int sl = base + __popcll(ms & below);
        if (same && sl < SCAP) sidx[sl] = (int)j;
    };
    const int64_t plo = unord64(mm[0]), phi = unord64(mm[1]);
    if ((uint64_t)(phi - plo) < 0xFFFFull) {  // packed uint16 labels, 8 per 16-byte load
        if (qpid >= plo && qpid <= phi) {
            const uint16_t key = (uint16_t)(qpid - plo);
            constexpr int U1 = 8, CH = 2048 * U1;  // U1: 16-byte label loads in flight per thread
            const int64_t nch = (G + CH - 1) / CH;
            const int64_t c0 = (q * 37) % nch;
            const int64_t n8 = (G + 7) / 8;
            for (int64_t c = 0; c < nch; c++) {
                int64_t v0 = ((c0 + c) % nch) * (CH / 8);
                uint4 w[U1];
#pragma unroll
                for (int u = 0; u < U1; u++) {
                    const int64_t v = v0 + u * 256 + tid;
                    w[u] = v < n8 ? ((const uint4*)pk)[v] : make_uint4(~0u, ~0u, ~0u, ~0u);
                }
                // 8 labels per lane tested at once: a 16-bit half of x = d ^ (key | key << 16)
                // is zero iff that label is the key (padding 0xFFFF never equals a key); one
                // ballot per 8 labels, the per-label ballots only where some lane hit
                const uint32_t kk = (uint32_t)key * 0x10001u;
#pragma unroll
                for (int u = 0; u < U1; u++) {
                    const int64_t jb = (v0 + u * 256 + tid) * 8;
                    const uint32_t d[4] = {w[u].x ^ kk, w[u].y ^ kk, w[u].z ^ kk, w[u].w ^ kk};
                    bool any = false;
#pragma unroll
                    for (int e = 0; e < 4; e++) any = any || (d[e] & 0xFFFFu) == 0u || (d[e] >> 16) == 0u;
                    if (!__ballot(any)) continue;
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const bool same = ((d[e >> 1] >> (16 * (e & 1))) & 0xFFFFu) == 0u;
                        if (__ballot(same)) take(same, jb + e);
                    }
                }
            }
        }
    } else {
        constexpr int U1 = 4, CH = 256 * U1;
        const int64_t nch = (G + CH - 1) / CH;
        const int64_t c0 = (q * 37) % nch;
        for (int64_t c = 0; c < nch; c++) {
            const int64_t j0 = ((c0 + c) % nch) * CH;
            int64_t pid[U1];
#pragma unroll
            for (int u = 0; u < U1; u++) {
                const int64_t j = j0 + u * 256 + tid;
                pid[u] = j < G ? gp[j] : qpid + 1;
            }
#pragma unroll
            for (int u = 0; u < U1; u++) {
                const bool same = pid[u] == qpid;
                if (__ballot(same)) take(same, j0 + u * 256 + tid);
            }
        }
    }
    __syncthreads();
    const int ns = s_ns;
    // ---- split them into positives (other camera) and junk (same camera, removed,
    // evaluate.py:55-56), their cameras and distances loaded in one round trip
    if (ns <= SCAP) {
        for (int t = tid; t < ns; t += 256) {
            const int j = sidx[t];
            const int64_t cam = gc[j];
            const float v = row[j];
            if (cam == qcam) {
                const int sl = atomicAdd(&s_nj, 1);
                if (sl < EVW_MAXJ) { ji[sl] = j; jv[sl] = v; }
            } else {
                const int sl = atomicAdd(&s_m, 1);
                if (sl < EVW_MAXP) { pi[sl] = j; pv[sl] = v; }
            }
        }
    }
    __syncthreads();
    const int m = s_m, nj = s_nj;
    if (ns > SCAP || m > EVW_MAXP || nj > EVW_MAXJ) {  // eval_rows_kernel (large lists) takes it
        if (tid == 0) {
            valid[q] = 2;
            *large = 1;
        }
        return;
    }
    if (tid == 0) nkept[q] = G - nj;
    if (m == 0) {
        if (tid == 0) { valid[q] = 0; first[q] = -1; ap[q] = 0.0; }
        return;
    }
    // ---- sort the positives by (value, index)
    int P = 1;
    while (P < m) P <<= 1;
    for (int t = m + tid; t < P; t += 256) {
        pv[t] = __builtin_inff();
        pi[t] = 0x7fffffff;
    }
    for (int t = tid; t <= m; t += 256) hist[t] = 0;
    __syncthreads();
    bitonic_sort_kv(pv, pi, P);
    // ---- pass 2: bin every item of the row by the number of positives before it.  A
    // bucket table narrows each item's candidates: t(x) = clamp(floor((x - v_0) * T /
    // (v_last - v_0)), 0, T-1) is monotone in x (the same float operations for every x), so
    // positives in buckets below t(x) are all smaller, those above all larger, and only the
    // positives of bucket t(x) need the exact (value, index) compare.  The table entry carries
    // the bucket's first positive value: with at most one positive in the bucket and no tie
    // with it, b = S[t] + (v_first < x) — branch-free, one 8-byte LDS read per item; buckets
    // of two or more positives and exact ties take the (value, index) walk, per wave only when
    // some lane needs it.
    const float lv = pv[m - 1];
    const int li = pi[m - 1];
    const float v0 = pv[0];
    const int T = 8 * P < EVW_T ? (8 * P > 64 ? 8 * P : 64) : EVW_T;  // ~8 buckets per positive
    // t(x) = floor(med3(x * scale - v_0 * scale, 0, T-1)): one fma, one med3, one convert
    // per item; when the positives tie (scale inf / NaN) every item goes to bucket 0 and the
    // exact compares decide
    float scale = (float)T / (lv - v0);
    if (!(scale <= 3.0e38f)) scale = 0.0f;
    const float c0 = -v0 * scale, tmax = (float)(T - 1);
    auto bucket_of = [&](float x) {  // med3 clamps to [0, T-1] (NaN to 0 or T-1), truncation floors
        return (int)__builtin_amdgcn_fmed3f(__builtin_fmaf(x, scale, c0), 0.0f, tmax);
    };
    constexpr int MULTI = 1 << 16;
    for (int t = tid; t <= T; t += 256) {  // S[t] = #{k : t(pv_k) < t}; n_t positives in bucket t
        int lo = m, n = 0;
        if (t < T) {
            lo = 0;
            int hi = m;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (bucket_of(pv[mid]) < t) lo = mid + 1; else hi = mid;
            }
            int lo2 = lo, hi2 = m;
            while (lo2 < hi2) {
                const int mid = (lo2 + hi2) >> 1;
                if (bucket_of(pv[mid]) <= t) lo2 = mid + 1; else hi2 = mid;
            }
            n = lo2 - lo;
        }
        bucket[t] = make_int2(n > 0 ? __float_as_int(pv[lo]) : 0x7f800000, lo | (n > 1 ? MULTI : 0));
    }
    __syncthreads();
    // b for an item of bucket t with entry e: the exact (value, index) walk over the bucket
    auto walk = [&](int t, int2 e, float v, int j) {
        int b = e.y & 0xFFFF;
        const int end = bucket[t + 1].y & 0xFFFF;
        while (b < end && key_less(pv[b], pi[b], v, j)) b++;
        return b;
    };
    auto bin = [&](float v, int j) {
        // after the last positive (b = m, not needed); NaN sorts last (np.argsort):
        // key_less(lv, li, v, j) || v != v, with the NaN test folded into !(v <= lv)
        if (!(v <= lv) || (v == lv && j > li)) return;
        const int t = bucket_of(v);
        atomicAdd(&hist[walk(t, bucket[t], v, j)], 1);
    };
    if (tid < h) bin(row[tid], tid);
    int* const mytrash = &trash[tid];
    for (int g0 = 0; g0 < nv; g0 += 256 * U2) {
        load_chunk(g0);
#pragma unroll
        for (int u = 0; u < U2; u++) {
            const int g = g0 + u * 256 + tid;
            const float x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            int tb[4];
            bool ok[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                // items after the last positive are not needed (b = m); NaN sorts last
                // (np.argsort) and fails x <= lv.  An item tied with the last positive's value
                // but after it (x == lv, j > li) is binned: it gets b = m, a count in hist[m]
                // that no rank reads
                ok[k] = (g < nv) & (x[k] <= lv);
                tb[k] = bucket_of(x[k]);
            }
            int2 se[4];
#pragma unroll
            for (int k = 0; k < 4; k++) se[k] = bucket[tb[k]];
            int b[4];
            bool sl[4], slow = false;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float vf = __int_as_float(se[k].x);
                b[k] = (se[k].y & 0xFFFF) + (vf < x[k] ? 1 : 0);
                sl[k] = ok[k] & ((se[k].y >= MULTI) | (vf == x[k]));
                slow = slow | sl[k];
            }
            if (__ballot(slow)) {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (sl[k]) b[k] = walk(tb[k], se[k], x[k], h + g * 4 + k);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) atomicAdd(ok[k] ? &hist[b[k]] : mytrash, 1);
        }
    }
    for (int64_t j = h + (int64_t)nv * 4 + tid; j < G; j += 256) bin(row[j], (int)j);
    __syncthreads();
    // ---- ranks (wave 0): inclusive scan of hist, minus the item itself and the junk before it
    if (tid < 64) {
        int carry = 0;
        for (int c0 = 0; c0 < m; c0 += 64) {
            const int k = c0 + lane;
            int v = k < m ? hist[k] : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(v, o, 64);
                if (lane >= o) v += t;
            }
            const int incl = v + carry;
            carry = __shfl(incl, 63, 64);
            if (k < m) {
                const float pvk = pv[k];
                const int pik = pi[k];
                int jb = 0;
                for (int t = 0; t < nj; t++) jb += key_less(jv[t], ji[t], pvk, pik);
                hist[k] = incl - 1 - jb;  // rank_k (0-based position among the kept items)
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const int* rk = hist;
        const double sum =
            m <= 64 ? pairwise_tree_par(lane < m ? rk[lane] : 0, rk,
                                        [](int t, int r) { return (double)(t + 1) / (double)(r + 1); }, m, G - nj)
                    : pairwise_tree_wave(rk, [&](int t) { return (double)(t + 1) / (double)(rk[t] + 1); }, m, G - nj,
                                         (uint32_t*)pv, pi, tvals, tops);  // pv / pi are free now
        if (lane == 0) {
            valid[q] = 1;
            first[q] = rk[0];
            ap[q] = sum / (double)m;
        }
    }
}

constexpr int EV_MAXP = 2048;

// Fallback for the queries eval_rows_wg_kernel left (valid == 2: more than EVW_MAXP
// positives or EVW_MAXJ junk items): one workgroup per query, up to EV_MAXP positives in
// LDS.  Positives are collected and sorted; every other kept gallery item is binned by how
// many positives precede it (binary search).  A query with more positives than that is
// marked valid = 3 and evaluated by the kernel's LAST workgroup to finish, with the same
// code on scratch arrays in the call's workspace sized for the whole gallery (EvScratch):
// no capacity limit, as in the reference.
struct EvLargeLds {
    float pv[EV_MAXP];
    int pi[EV_MAXP];
    int hist[EV_MAXP + 1];
    int64_t rk[EV_MAXP];
    double rv[EV_MAXP];
    int s_m, s_junk;
    PwFrame pw[PW_DEPTH];
};

struct EvScratch {  // arrays of the large-list evaluation (LDS, or global memory)
    float* pv;
    int* pi;
    int* hist;
    int64_t* rk;
    double* rv;
    int64_t cap;  // positives the arrays hold (pv / pi hold pow2_ceil(cap))
};

// returns false (and sets nothing) when the query has more than S.cap positives
__device__ bool eval_row_large(int64_t q, const float* __restrict__ dist, int64_t G, int64_t ld,
                               const int64_t* __restrict__ qp, const int64_t* __restrict__ gp,
                               const int64_t* __restrict__ qc, const int64_t* __restrict__ gc,
                               int32_t* __restrict__ valid, int64_t* __restrict__ first, double* __restrict__ ap,
                               int64_t* __restrict__ nkept, const EvScratch& S, EvLargeLds& L) {
    float* pv = S.pv;
    int* pi = S.pi;
    int* hist = S.hist;
    int64_t* rk = S.rk;
    double* rv = S.rv;
    int& s_m = L.s_m;
    int& s_junk = L.s_junk;
    PwFrame* pw = L.pw;
    const float* row = dist + q * ld;
    const int64_t qpid = qp[q], qcam = qc[q];
    if (threadIdx.x == 0) { s_m = 0; s_junk = 0; }
    __syncthreads();
    for (int64_t j = threadIdx.x; j < G; j += blockDim.x) {
        if (gp[j] == qpid) {
            if (gc[j] == qcam) atomicAdd(&s_junk, 1);
            else {
                int p = atomicAdd(&s_m, 1);
                if (p < S.cap) { pv[p] = row[j]; pi[p] = (int)j; }
            }
        }
    }
    __syncthreads();
    const int m = s_m;
    if (m > S.cap) return false;
    const int P = pow2_ceil(m < 2 ? 2 : m);
    for (int t = m + threadIdx.x; t < P; t += blockDim.x) { pv[t] = __builtin_inff(); pi[t] = 0x7fffffff; }
    for (int t = threadIdx.x; t <= m; t += blockDim.x) hist[t] = 0;
    __syncthreads();
    bitonic_sort_kv(pv, pi, P);
    for (int64_t j = threadIdx.x; j < G; j += blockDim.x) {
        if (gp[j] == qpid) continue;  // positives counted separately, junk removed
        const float v = row[j];
        int lo = 0, hi = m;
        while (lo < hi) {
            int mid = (lo + hi) >> 1;
            if (key_less(pv[mid], pi[mid], v, (int)j)) lo = mid + 1; else hi = mid;
        }
        if (lo < m) atomicAdd(&hist[lo], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t n = G - s_junk;
        nkept[q] = n;
        valid[q] = 1;
        int64_t cum = 0;
        for (int k = 0; k < m; k++) {
            cum += hist[k];
            rk[k] = k + cum;
            rv[k] = (double)(k + 1) / (double)(rk[k] + 1);
        }
        first[q] = rk[0];
        ap[q] = pairwise_sparse([&](int t) { return rk[t]; }, [&](int t) { return rv[t]; }, m, n, pw) / (double)m;
    }
    __syncthreads();
    return true;
}

// Grid-stride over the queries (a few workgroups per CU instead of one launch-slot per query);
// the last workgroup to finish takes the queries marked valid = 3.  A workgroup that marked
// one counts it (hugecount) and issues a release fence before its arrival; the last arrival
// issues an acquire fence and, only when the count is non-zero, scans valid[] in parallel —
// nothing of this runs unless eval_rows_wg_kernel deferred a query (*large).
__global__ __launch_bounds__(256) void eval_rows_kernel(
    const float* __restrict__ dist, int64_t Q, int64_t G, int64_t ld, const int64_t* __restrict__ qp,
    const int64_t* __restrict__ gp, const int64_t* __restrict__ qc, const int64_t* __restrict__ gc,
    int32_t* __restrict__ valid, int64_t* __restrict__ first, double* __restrict__ ap,
    int64_t* __restrict__ nkept, const int32_t* __restrict__ large, unsigned int* __restrict__ arrivals,
    unsigned int* __restrict__ hugecount, EvScratch huge) {
    if (*large == 0) return;  // no query left for this kernel (the common case: one load per workgroup)
    __shared__ EvLargeLds L;
    __shared__ int s_last, s_mark;
    __shared__ unsigned int s_cnt;
    const EvScratch lds{L.pv, L.pi, L.hist, L.rk, L.rv, EV_MAXP};
    if (threadIdx.x == 0) s_mark = 0;
    __syncthreads();
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        if (valid[q] != 2) continue;  // uniform per workgroup
        if (!eval_row_large(q, dist, G, ld, qp, gp, qc, gc, valid, first, ap, nkept, lds, L) && threadIdx.x == 0) {
            valid[q] = 3;
            s_mark = 1;
            atomicAdd(hugecount, 1u);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s_mark) __threadfence();
        const unsigned int prev = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev == gridDim.x - 1;
        s_cnt = 0;
        if (s_last) {
            __threadfence();
            s_cnt = __hip_atomic_load(hugecount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (!s_last || s_cnt == 0) return;
    __shared__ int flag[256];
    for (int64_t q0 = 0; q0 < Q; q0 += blockDim.x) {
        const int64_t q = q0 + threadIdx.x;
        const bool h = q < Q && valid[q] == 3;
        flag[threadIdx.x] = h;
        if (!__syncthreads_or(h)) continue;
        for (int t = 0; t < (int)blockDim.x; t++)
            if (flag[t]) eval_row_large(q0 + t, dist, G, ld, qp, gp, qc, gc, valid, first, ap, nkept, huge, L);
        __syncthreads();
    }
}

// ------------------------------------------------- the last stage of the matrix-free scoring
// evalfeat.hip counted, per query, hist[b] = kept gallery items (the matches among them) with
// exactly b matches before them, over every gallery block; removed items were never counted.  One
// wave per query scans it into the kept-ranks, rank_t = sum_{b <= t} hist[b] - 1, and sums the AP
// with the summers above exactly as the two eval_rows kernels do: up to EVW_MAXP matches with the
// ranks in LDS (pairwise_tree_par / pairwise_tree_wave, eval_rows_wg_kernel's choice), more with
// the ranks written over hist and pairwise_sparse (eval_row_large's).
__global__ __launch_bounds__(64) void evf_finish_kernel(const int32_t* __restrict__ pos_cnt, int32_t* hist_all,
                                                        const int32_t* __restrict__ junk_cnt, int cap,
                                                        int64_t G_total, int32_t* __restrict__ overflow,
                                                        int32_t* __restrict__ valid, int64_t* __restrict__ first,
                                                        int64_t* __restrict__ last, int32_t* __restrict__ npos,
                                                        double* __restrict__ ap, int64_t* __restrict__ nkept) {
    __shared__ int rks[EVW_MAXP];
    __shared__ uint32_t path[EVW_MAXP];
    __shared__ int dep[EVW_MAXP];
    __shared__ double tvals[AP_STACK];
    __shared__ int tops[AP_STACK];
    __shared__ PwFrame pw[PW_DEPTH];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int m = pos_cnt[q];
    const int64_t n = G_total - junk_cnt[q];
    int32_t* hist = hist_all + q * ((int64_t)cap + 1);
    if (m > cap || m == 0) {  // a list that did not fit; no match
        if (lane == 0) {
            valid[q] = m ? -1 : 0;
            first[q] = -1;
            ap[q] = 0.0;
            nkept[q] = n;
            if (last) last[q] = -1;
            if (npos) npos[q] = m;
            if (m) *overflow = 1;
        }
        return;
    }
    const bool lds = m <= EVW_MAXP;
    int carry = 0;
    for (int c0 = 0; c0 < m; c0 += 64) {
        const int k = c0 + lane;
        int v = k < m ? hist[k] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(v, o, 64);
            if (lane >= o) v += t;
        }
        const int incl = v + carry;
        carry = __shfl(incl, 63, 64);
        if (k < m) {
            if (lds) rks[k] = incl - 1;
            else hist[k] = incl - 1;
        }
    }
    __syncthreads();  // one wave: the ranks are visible to every lane
    double sum;
    int64_t r0, rl;
    if (lds) {
        const int* rk = rks;
        sum = m <= 64 ? pairwise_tree_par(lane < m ? rk[lane] : 0, rk,
                                          [](int t, int r) { return (double)(t + 1) / (double)(r + 1); }, m, n)
                      : pairwise_tree_wave(rk, [&](int t) { return (double)(t + 1) / (double)(rk[t] + 1); }, m, n,
                                           path, dep, tvals, tops);
        r0 = rk[0];
        rl = rk[m - 1];
    } else {
        sum = 0.0;
        if (lane == 0)
            sum = pairwise_sparse([&](int t) { return (int64_t)hist[t]; },
                                  [&](int t) { return (double)(t + 1) / (double)(hist[t] + 1); }, m, n, pw);
        r0 = hist[0];
        rl = hist[m - 1];
    }
    if (lane == 0) {
        valid[q] = 1;
        first[q] = r0;
        ap[q] = sum / (double)m;
        nkept[q] = n;
        if (last) last[q] = rl;
        if (npos) npos[q] = m;
    }
}

int evf_finish_launch(const int32_t* pos_cnt, int32_t* hist, const int32_t* junk_cnt, int64_t Q, int cap,
                      int64_t G_total, int32_t* overflow, int32_t* valid, int64_t* first, int64_t* last,
                      int32_t* npos, double* ap, int64_t* nkept, hipStream_t s) {
    RM_REQUIRE(Q >= 0 && Q < (1ll << 31) && G_total > 0 && G_total < (1ll << 31), "evf_finish: bad shape");
    RM_REQUIRE(cap >= 1, "evf_finish: need cap >= 1");
    RM_REQUIRE(pos_cnt != nullptr && hist != nullptr && junk_cnt != nullptr && overflow != nullptr,
               "evf_finish: pos_cnt, hist, junk_cnt and overflow required");
    RM_REQUIRE(valid != nullptr && first != nullptr && ap != nullptr && nkept != nullptr,
               "evf_finish: valid, first, ap and nkept required");
    if (Q == 0) return OK;
    hipLaunchKernelGGL(evf_finish_kernel, dim3((unsigned)Q), dim3(64), 0, s, pos_cnt, hist, junk_cnt, cap, G_total,
                       overflow, valid, first, last, npos, ap, nkept);
    RM_LAUNCHED();
    return OK;
}

}  // namespace reidmi

using namespace reidmi;

// workspace: [0, 256) min/max + arrival counter | packed labels (G8 uint16) | large-list
// scratch for one query of up to G positives: pv, pi (pow2_ceil(G) each), hist (G + 1),
// rk, rv (G each)
static int64_t ev_pow2(int64_t G) {
    int64_t p = 2;
    while (p < G) p <<= 1;
    return p;
}
static int64_t ev_lab_bytes(int64_t G) { return ((G + 7) / 8 * 8) * 2; }
static int64_t ev_huge_off(int64_t G) { return (256 + ev_lab_bytes(G) + 15) / 16 * 16; }
static int64_t ev_ws_bytes(int64_t G) {
    const int64_t P2 = ev_pow2(G);
    return ev_huge_off(G) + P2 * 8 + ((G + 1) * 4 + 7) / 8 * 8 + G * 16;
}

REIDMI_API int64_t reidmi_eval_rows_workspace_bytes(int64_t G) { return G > 0 ? ev_ws_bytes(G) : -1; }

REIDMI_API int reidmi_eval_rows(const float* dist, int64_t Q, int64_t G, int64_t ldd, const int64_t* q_pids,
                                const int64_t* g_pids, const int64_t* q_cams, const int64_t* g_cams, int32_t* valid,
                                int64_t* first, double* ap, int64_t* nkept, int32_t* overflow, void* ws_,
                                int64_t ws_bytes, void* stream) {
    RM_REQUIRE(Q >= 0 && G > 0 && ldd >= G && G < 0x7fffffff, "eval_rows: bad shape");
    RM_REQUIRE(overflow != nullptr, "eval_rows: overflow flag pointer required");
    RM_REQUIRE(((uintptr_t)dist & 3) == 0, "eval_rows: dist must be 4-byte aligned");
    RM_REQUIRE(ws_ != nullptr && ((uintptr_t)ws_ & 15) == 0 && ws_bytes >= ev_ws_bytes(G),
               "eval_rows: workspace (reidmi_eval_rows_workspace_bytes, 16-byte aligned) required");
    if (Q == 0) return OK;
    RM_REQUIRE(Q < (1ll << 31), "eval_rows: too many queries");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* mm = (unsigned long long*)ws_;
    uint16_t* pk = (uint16_t*)((char*)ws_ + 256);
    const int64_t G8 = (G + 7) / 8 * 8;
    if (G <= EV_PREP1_MAX) {
        hipLaunchKernelGGL(ev_prep1_kernel, dim3(1), dim3(1024), 0, s, g_pids, G, G8, mm, pk, overflow);
        RM_LAUNCHED();
    } else {
        hipLaunchKernelGGL(ev_minmax_init_kernel, dim3(1), dim3(1), 0, s, mm, overflow);
        RM_LAUNCHED();
        hipLaunchKernelGGL(ev_minmax_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(G, 256), 1024)), dim3(256), 0,
                           s, g_pids, G, mm);
        RM_LAUNCHED();
        hipLaunchKernelGGL(ev_pack_kernel, dim3(ceil_div(G8, 256)), dim3(256), 0, s, g_pids, G, G8,
                           (const unsigned long long*)mm, pk);
        RM_LAUNCHED();
    }
    hipLaunchKernelGGL(eval_rows_wg_kernel, dim3((unsigned)Q), dim3(256), 0, s, dist, G, ldd, q_pids, g_pids, q_cams,
                       g_cams, (const unsigned long long*)mm, (const uint16_t*)pk, valid, first, ap, nkept,
                       (int32_t*)(mm + 3));
    RM_LAUNCHED();
    EvScratch huge{};
    {
        char* h = (char*)ws_ + ev_huge_off(G);
        const int64_t P2 = ev_pow2(G);
        huge.pv = (float*)h;
        huge.pi = (int*)(h + P2 * 4);
        huge.hist = (int*)(h + P2 * 8);
        huge.rk = (int64_t*)(h + P2 * 8 + ((G + 1) * 4 + 7) / 8 * 8);
        huge.rv = (double*)((char*)huge.rk + G * 8);
        huge.cap = G;
    }
    hipLaunchKernelGGL(eval_rows_kernel, dim3((unsigned)std::min<int64_t>(Q, 512)), dim3(256), 0, s, dist, Q, G, ldd,
                       q_pids, g_pids, q_cams, g_cams, valid, first, ap, nkept, (const int32_t*)(mm + 3),
                       (unsigned int*)(mm + 2), (unsigned int*)(mm + 2) + 1, huge);
    RM_LAUNCHED();
    return OK;
}
