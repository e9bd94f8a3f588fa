// cluster.hip — exact DBSCAN over the rows of x from the features, without the N x N matrix
// (reidmi_dbscan_f32; include/reidmi.h has the contract).
//
// Three passes over the distance tiles of x against itself, each the mainloop of the distance
// kernels (distance.h), so d(i, j) has reidmi_distmat_f32's bits, and none stores a tile:
//   count    hits per row (d <= eps, or the diagonal) -> counts; then core = counts >= min_samples
//   union    every core pair within eps joins its two trees in parent[] (lock-free, cluster.h)
//   border   every non-core row takes the smallest root among its core columns within eps
// and between / after them the O(N) kernels: init, compress (every parent becomes its root), the
// scan of the root flags into cluster numbers, and the labels.
//
// Why the result does not depend on scheduling.  A tree is only ever changed at its root r, by
// atomicCAS(&parent[r], r, s) with s < r the root of the other tree: an entry changes once, from
// "itself" to something smaller, and the root of a tree is always its lowest index.  Whatever
// order the unions land in, the trees at the end are the connected components of the core graph
// and each one's root is the component's lowest core index.  A read in find may be stale only in
// one way (it still sees "itself" where the entry was hooked meanwhile); the CAS then fails,
// returns the entry's value, and the walk goes on from there.  Every retry follows a strictly
// smaller index, nobody waits for anybody.  Counts are integer sums, border roots integer minima.
#include "backend.h"
#include "cluster.h"
#include "distance.h"

namespace reidmi {

// distance.h's band-and-range walk: a workgroup owns one 128-row band and one contiguous column
// range [c0, c1) and walks it in 128-column tiles.  Row state in LDS.  LDS: 33 024 B of operand
// stages + 1.5 KB of row state: four workgroups per CU.
//   COUNT   every lane keeps the count of one row of its wave's quadrant (32 rows per half-wave,
//           32 lanes per half-wave) in one register: the hits of a row are the set bits of its
//           half of a ballot.  One LDS add per lane and one global add per row at the range's end.
//   UNION   rows and columns are core points; the pair (i, j) is joined from the tile that holds it
//           with i < j (the distance bits are symmetric).  A lane's column keeps its last root.
//   BORDER  rows are non-core, columns core; the row's minimum goes through the half-wave and LDS,
//           one global atomicMin per row at the range's end.
// UNION and BORDER skip a tile without a core column before its mainloop, and the whole range when
// the band has no row of their kind.
template <bool PIPE, int PASS>
__global__ __launch_bounds__(256, DM2_MINWG) void dbs_tile_kernel(
    const float* __restrict__ x, const float* __restrict__ xx, int64_t N, int64_t D, int64_t ldx, int64_t range_len,
    float eps, const uint8_t* __restrict__ core, int32_t* __restrict__ counts, int32_t* parent,
    int32_t* __restrict__ border) {
    __shared__ float smem[DM_SMEM];
    __shared__ float s_xx[DM_BM];
    __shared__ int s_row[DM_BM];  // COUNT: hits; UNION / BORDER: the row takes part
    __shared__ int s_min[DM_BM];  // BORDER: smallest root so far
    const DmThread t = dm_thread();
    const int tid = t.tid, lane = t.lane, wm = t.wm, wn = t.wn;
    const DmWalk w = dm_walk(N, N, range_len);
    const int64_t bm = w.bm, c0 = w.c0, c1 = w.c1;
    bool mine = false;
    if (tid < DM_BM) {
        const bool in = bm + tid < N;
        s_xx[tid] = in ? xx[bm + tid] : 0.0f;
        s_min[tid] = DBS_NONE;
        if constexpr (PASS == DBS_COUNT) s_row[tid] = 0;
        else {
            mine = in && (core[bm + tid] != 0) == (PASS == DBS_UNION);
            s_row[tid] = mine;
        }
    }
    if constexpr (PASS == DBS_COUNT) __syncthreads();
    else if (!__syncthreads_or(mine)) return;
    int my_hits = 0;  // COUNT: row (lane & 31) of the quadrant's half (lane >> 5)
    for (int64_t bn = c0; bn < c1; bn += DM_BN) {
        if constexpr (PASS != DBS_COUNT) {
            const bool cj = tid < DM_BN && bn + tid < c1 && core[bn + tid] != 0;
            if (!__syncthreads_or(cj)) continue;
        }
        f32x16 acc[2][2];
        dm_acc_zero(acc);
        dm_tile<PIPE>(t, x, x, N, c1, D, ldx, ldx, bm, bn, smem, acc);
        int64_t j[2];
        float xxj[2];
        bool jok[2];
        int rj[2];
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            j[nt] = bn + dm_lane_col(wn, nt, lane);
            jok[nt] = j[nt] < c1;
            xxj[nt] = jok[nt] ? xx[j[nt]] : 0.0f;
            if constexpr (PASS != DBS_COUNT) jok[nt] = jok[nt] && core[j[nt]] != 0;
            rj[nt] = DBS_NONE;
            if constexpr (PASS == DBS_UNION) rj[nt] = (int)j[nt];
            if constexpr (PASS == DBS_BORDER) rj[nt] = jok[nt] ? parent[j[nt]] : DBS_NONE;  // final roots
        }
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int il = dm_lane_row(wm, mt, r, lane);
                const int64_t i = bm + il;
                bool hit[2];
#pragma unroll
                for (int nt = 0; nt < 2; nt++) {
                    const float v = dm_value(acc[mt][nt][r], s_xx[il], xxj[nt]);
                    hit[nt] = jok[nt] && (v <= eps || (PASS == DBS_COUNT && i == j[nt]));
                }
                if constexpr (PASS == DBS_COUNT) {
                    // rows past N collect hits too; they are dropped when the counts are written
                    const unsigned long long m0 = __ballot(hit[0]), m1 = __ballot(hit[1]);
                    const int lo = __popc((unsigned)m0) + __popc((unsigned)m1);
                    const int hi = __popc((unsigned)(m0 >> 32)) + __popc((unsigned)(m1 >> 32));
                    if ((lane & 31) == mt * 16 + r) my_hits += lane < 32 ? lo : hi;
                } else if constexpr (PASS == DBS_UNION) {
                    if (!s_row[il]) continue;
#pragma unroll
                    for (int nt = 0; nt < 2; nt++)
                        if (hit[nt] && i < j[nt]) rj[nt] = dbs_union(parent, (int)i, rj[nt]);
                } else {
                    int m = DBS_NONE;
                    if (s_row[il]) {
                        if (hit[0]) m = rj[0];
                        if (hit[1] && rj[1] < m) m = rj[1];
                    }
                    if (__ballot(m != DBS_NONE) == 0) continue;
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) {  // the 32 lanes of a half-wave share the row
                        const int u = __shfl_xor(m, o, 64);
                        m = u < m ? u : m;
                    }
                    if ((lane & 31) == 0 && m != DBS_NONE) atomicMin(&s_min[il], m);
                }
            }
    }
    if constexpr (PASS == DBS_COUNT) {
        // lane l holds row mt = (l & 31) >> 4, r = l & 15 of its half
        atomicAdd(&s_row[dm_lane_row(wm, (lane & 31) >> 4, lane & 15, lane)], my_hits);
        __syncthreads();
        if (tid < DM_BM && bm + tid < N && s_row[tid] != 0) atomicAdd(&counts[bm + tid], s_row[tid]);
    } else if constexpr (PASS == DBS_BORDER) {
        __syncthreads();
        if (tid < DM_BM && bm + tid < N && s_min[tid] != DBS_NONE) atomicMin(&border[bm + tid], s_min[tid]);
    }
}

// ------------------------------------------------------------------- the O(N) kernels
__global__ __launch_bounds__(256) void dbs_init_kernel(const int32_t* __restrict__ counts, int64_t N, int min_samples,
                                                       uint8_t* __restrict__ core, int32_t* __restrict__ parent,
                                                       int32_t* __restrict__ border) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    core[i] = counts[i] >= min_samples;
    parent[i] = (int)i;
    border[i] = DBS_NONE;
}

// Every entry becomes its tree's root.  An entry overwritten while another thread walks through
// it holds either its parent or its root: both lie on the way to the same root.
__global__ __launch_bounds__(256) void dbs_compress_kernel(int32_t* parent, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int r = dbs_find(parent, (int)i);
    if (r != (int)i) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Cluster numbers: the exclusive scan of flag[i] = (i is a core point and its own root), in three
// steps: the sum of every DBS_SCAN-entry block, the exclusive scan of those sums by one workgroup,
// and the scan inside every block on top of its offset.
constexpr int DBS_SCAN_U = 8, DBS_SCAN = 256 * DBS_SCAN_U;

__device__ __forceinline__ int dbs_flag(const uint8_t* core, const int32_t* parent, int64_t i, int64_t N) {
    return i < N && core[i] != 0 && parent[i] == (int)i;
}

// Exclusive scan of one value per thread over the 256 threads; *total gets the sum.
__device__ __forceinline__ int dbs_block_scan(int v, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();  // s_wave is free (a previous call's reads are over)
    if (lane == 63) s_wave[wid] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int sw = s_wave[w];
        before += w < wid ? sw : 0;
        all += sw;
    }
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(256) void dbs_scan_sums_kernel(const uint8_t* __restrict__ core,
                                                            const int32_t* __restrict__ parent, int64_t N,
                                                            int32_t* __restrict__ bsum) {
    __shared__ int s_wave[4];
    const int64_t i0 = (int64_t)blockIdx.x * DBS_SCAN + (int64_t)threadIdx.x * DBS_SCAN_U;
    int v = 0;
#pragma unroll
    for (int u = 0; u < DBS_SCAN_U; u++) v += dbs_flag(core, parent, i0 + u, N);
    int total;
    dbs_block_scan(v, s_wave, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void dbs_scan_offsets_kernel(int32_t* bsum, int64_t nb,
                                                               int32_t* __restrict__ n_clusters) {
    __shared__ int s_wave[4];
    int carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        const int v = b < nb ? bsum[b] : 0;
        int total;
        const int ex = dbs_block_scan(v, s_wave, &total);
        if (b < nb) bsum[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *n_clusters = carry;
}

__global__ __launch_bounds__(256) void dbs_scan_number_kernel(const uint8_t* __restrict__ core,
                                                              const int32_t* __restrict__ parent, int64_t N,
                                                              const int32_t* __restrict__ bsum,
                                                              int32_t* __restrict__ number) {
    __shared__ int s_wave[4];
    const int64_t i0 = (int64_t)blockIdx.x * DBS_SCAN + (int64_t)threadIdx.x * DBS_SCAN_U;
    int f[DBS_SCAN_U], v = 0;
#pragma unroll
    for (int u = 0; u < DBS_SCAN_U; u++) {
        f[u] = dbs_flag(core, parent, i0 + u, N);
        v += f[u];
    }
    int total;
    int at = bsum[blockIdx.x] + dbs_block_scan(v, s_wave, &total);
#pragma unroll
    for (int u = 0; u < DBS_SCAN_U; u++) {
        if (f[u]) number[i0 + u] = at;  // read at the roots only
        at += f[u];
    }
}

__global__ __launch_bounds__(256) void dbs_labels_kernel(const uint8_t* __restrict__ core,
                                                         const int32_t* __restrict__ parent,
                                                         const int32_t* __restrict__ border,
                                                         const int32_t* __restrict__ number, int64_t N,
                                                         int32_t* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int root = core[i] ? parent[i] : border[i];
    labels[i] = root == DBS_NONE ? -1 : number[root];
}

// ------------------------------------------------------------------------- launchers
bool dbs_state(int64_t N, DbsState* w) {
    if (N < 1 || N >= (1ll << 31)) return false;
    const int64_t row = (N * 4 + 15) / 16 * 16;
    w->nb = (N + DBS_SCAN - 1) / DBS_SCAN;
    w->parent_off = 0;
    w->border_off = row;
    w->number_off = 2 * row;
    w->bsum_off = 3 * row;
    w->bytes = 3 * row + (w->nb * 4 + 15) / 16 * 16;
    return true;
}

int dbs_init_launch(const int32_t* counts, int64_t N, int min_samples, uint8_t* core, int32_t* parent, int32_t* border,
                    hipStream_t s) {
    hipLaunchKernelGGL(dbs_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, counts, N, min_samples,
                       core, parent, border);
    RM_LAUNCHED();
    return OK;
}

int dbs_compress_launch(int32_t* parent, int64_t N, hipStream_t s) {
    hipLaunchKernelGGL(dbs_compress_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, parent, N);
    RM_LAUNCHED();
    return OK;
}

int dbs_labels_launch(const uint8_t* core, const int32_t* parent, const int32_t* border, int32_t* number, int32_t* bsum,
                      int64_t nb, int64_t N, int32_t* n_clusters, int32_t* labels, hipStream_t s) {
    const dim3 rows((unsigned)((N + 255) / 256)), blocks((unsigned)nb);
    hipLaunchKernelGGL(dbs_scan_sums_kernel, blocks, dim3(256), 0, s, core, parent, N, bsum);
    RM_LAUNCHED();
    hipLaunchKernelGGL(dbs_scan_offsets_kernel, dim3(1), dim3(256), 0, s, bsum, nb, n_clusters);
    RM_LAUNCHED();
    hipLaunchKernelGGL(dbs_scan_number_kernel, blocks, dim3(256), 0, s, core, parent, N, (const int32_t*)bsum, number);
    RM_LAUNCHED();
    hipLaunchKernelGGL(dbs_labels_kernel, rows, dim3(256), 0, s, core, parent, border, (const int32_t*)number, N,
                       labels);
    RM_LAUNCHED();
    return OK;
}

// workspace: norms | the O(N) state (cluster.h)
static bool dbs_ws(int64_t N, int64_t D, DbsState* w, int64_t* bytes) {
    if (D < 1 || !dbs_state(N, w)) return false;
    *bytes = dm_norm_bytes(N, 0) + w->bytes;
    return true;
}

// The column ranges of a pass: distance.h's dm_walk_plan, the column tiles being the row bands.
template <int PASS>
static int dbs_pass_run(const float* x, const float* xx, int64_t N, int64_t D, int64_t ldx, float eps,
                        const uint8_t* core, int32_t* counts, int32_t* parent, int32_t* border, hipStream_t s) {
    const int64_t bands = (N + DM_BM - 1) / DM_BM;
    int64_t S, range_len;
    dm_walk_plan(bands, bands, &S, &range_len);
    RM_REQUIRE(bands * S < (1ll << 31), "dbscan: too many row bands for one launch");
    const dim3 grid((unsigned)(bands * S));
    RM_BOOL_SWITCH(dm2_ok(x, ldx, x, ldx, D), PIPE,
                   hipLaunchKernelGGL((dbs_tile_kernel<PIPE, PASS>), grid, dim3(256), 0, s, x, xx, N, D, ldx,
                                      range_len, eps, core, counts, parent, border));
    RM_LAUNCHED();
    return OK;
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int64_t reidmi_dbscan_workspace_bytes(int64_t N, int64_t D) {
    DbsState w;
    int64_t bytes;
    return dbs_ws(N, D, &w, &bytes) ? bytes : -1;
}

REIDMI_API int reidmi_dbscan_f32(const float* x, int64_t N, int64_t D, int64_t ldx, float eps, int min_samples,
                                 int32_t* labels, int32_t* counts, uint8_t* core, int32_t* n_clusters, void* ws,
                                 int64_t ws_bytes, void* stream) {
    RM_REQUIRE(N >= 1 && N < (1ll << 31) && D >= 1, "dbscan: bad shape (need 1 <= N < 2^31, D >= 1)");
    RM_REQUIRE(ldx >= D, "dbscan: the row pitch must be >= D");
    RM_REQUIRE(eps >= 0.0f && eps <= 3.402823466e+38f, "dbscan: eps must be finite and >= 0");
    RM_REQUIRE(min_samples >= 1, "dbscan: need min_samples >= 1");
    RM_REQUIRE(x != nullptr, "dbscan: features required");
    RM_REQUIRE(labels != nullptr && counts != nullptr && core != nullptr && n_clusters != nullptr,
               "dbscan: labels, counts, core and n_clusters required");
    DbsState w;
    int64_t bytes;
    RM_REQUIRE(dbs_ws(N, D, &w, &bytes) && ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= bytes,
               "dbscan: workspace (reidmi_dbscan_workspace_bytes, 16-byte aligned) required");
    hipStream_t s = (hipStream_t)stream;
    float* xx = (float*)ws;
    char* state = (char*)ws + (bytes - w.bytes);
    int32_t* parent = (int32_t*)(state + w.parent_off);
    int32_t* border = (int32_t*)(state + w.border_off);
    int32_t* number = (int32_t*)(state + w.number_off);
    int32_t* bsum = (int32_t*)(state + w.bsum_off);
    RM_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)N * 4, s));
    rows_sqnorm_launch(x, N, D, ldx, xx, s);
    RM_LAUNCHED();
    RM_TRY(dbs_pass_run<DBS_COUNT>(x, xx, N, D, ldx, eps, core, counts, parent, border, s));
    RM_TRY(dbs_init_launch(counts, N, min_samples, core, parent, border, s));
    RM_TRY(dbs_pass_run<DBS_UNION>(x, xx, N, D, ldx, eps, core, counts, parent, border, s));
    RM_TRY(dbs_compress_launch(parent, N, s));
    RM_TRY(dbs_pass_run<DBS_BORDER>(x, xx, N, D, ldx, eps, core, counts, parent, border, s));
    return dbs_labels_launch(core, parent, border, number, bsum, w.nb, N, n_clusters, labels, s);
}
