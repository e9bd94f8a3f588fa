// pairhist.hip — verification and open-set statistics from the features, without the Q x G
// matrix (reidmi_pair_stats_f32; include/reidmi.h has the contract).
//
// Per labelled (query, gallery item) pair: the bin of its distance under the caller's edges,
// counted apart for genuine and impostor pairs, and per query the nearest genuine and the nearest
// impostor item.  distance.h's band-and-range walk: the distance kernels' mainloop, so d(i, j)
// has reidmi_distmat_f32's bits, with an epilogue of its own; no tile is stored.
//
// Why the result does not depend on scheduling.  The histograms are integer sums: any order of the
// adds, in LDS or in global memory, gives the same counts.  A nearest item is the minimum of a
// packed 64-bit key (ordered distance bits, global index) that is unique per item; a minimum does
// not depend on the order either, and the in/out pair of a row only ever moves to a smaller key.
// So gallery blocks, ranges and ranks may be processed in any order.
#include "backend.h"
#include "distance.h"

namespace reidmi {

constexpr int PH_MAX_EDGES = 255, PH_BINS = PH_MAX_EDGES + 1;
// An LDS bin is 32 bits wide and a tile adds at most DM_BM * DM_BN = 2^14 to one: the bins are
// flushed to the 64-bit global counters at the range's end and after every PH_FLUSH_TILES tiles,
// so none holds more than 2^31.
constexpr int64_t PH_FLUSH_TILES = 1 << 17;
constexpr unsigned long long PH_NOKEY = ~0ull;  // no item: above every key (an index is < 2^31 - 1)

// The edges travel by value in the kernel arguments (no copy, no synchronisation): e[n..] = +inf.
struct PhEdges {
    float e[PH_BINS];
};

// fp32 bits as an unsigned integer in the order of fp32 `<`; -0.0 is made +0.0 first, so the two
// zeros tie (the distance kernel never yields -0.0: the sum of two squared norms is never -0.0).
__device__ __forceinline__ unsigned ph_ordered(float v) {
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ph_unordered(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// A workgroup owns one 128-row query band and one contiguous gallery range [c0, c1) of the block
// and walks it in 128-column tiles.  LDS beside the 33 024 B of operand stages: the edges (1 KB),
// the two histograms (2 KB), the row state (norm, pid, cam: 2.5 KB) and the two row minima (2 KB):
// 40 704 B, four workgroups per CU.
//   bin      b = #{t : edges[t] < d} by a branch-free binary search over the 256 padded edges in LDS
//   count    one LDS add per pair on hist[class][b]; one global 64-bit add per non-empty bin at the flush
//   nearest  a pair whose key is below the row's minimum in LDS lowers it (an LDS 64-bit min); after
//            the first tiles nearly every pair ends at the compare.  One global min per row and
//            class at the range's end, into the workspace; ph_finish_kernel merges it into the
//            caller's (dist, idx).
template <bool PIPE>
__global__ __launch_bounds__(256, DM2_MINWG) void ph_tile_kernel(
    const float* __restrict__ q, const float* __restrict__ g, const float* __restrict__ qq,
    const float* __restrict__ gg, int64_t Q, int64_t Gb, int64_t D, int64_t ldq, int64_t ldg, DmLabels lab,
    PhEdges edges, int64_t range_len, int64_t index_base, int64_t self_base,
    unsigned long long* __restrict__ hist_pos, unsigned long long* __restrict__ hist_neg,
    unsigned long long* __restrict__ key_pos, unsigned long long* __restrict__ key_neg) {
    __shared__ float smem[DM_SMEM];
    __shared__ float s_edges[PH_BINS];
    __shared__ unsigned s_hist[2][PH_BINS];         // [0] impostor, [1] genuine
    __shared__ unsigned long long s_key[2][DM_BM];  // likewise
    __shared__ float s_qq[DM_BM];
    __shared__ int64_t s_qp[DM_BM], s_qc[DM_BM];
    const DmThread t = dm_thread();
    const int tid = t.tid, lane = t.lane, wm = t.wm, wn = t.wn;
    const bool cams = lab.qc != nullptr;  // qc, gc: both or neither
    const DmWalk w = dm_walk(Q, Gb, range_len);
    const int64_t bm = w.bm, c0 = w.c0, c1 = w.c1;
    const int nq = Q - bm < DM_BM ? (int)(Q - bm) : DM_BM;
    s_edges[tid] = edges.e[tid];
    s_hist[0][tid] = 0;
    s_hist[1][tid] = 0;
    s_key[tid >> 7][tid & (DM_BM - 1)] = PH_NOKEY;
    if (tid < DM_BM) {
        const bool in = tid < nq;
        s_qq[tid] = in ? qq[bm + tid] : 0.0f;
        s_qp[tid] = in ? lab.qp[bm + tid] : 0;
        s_qc[tid] = in && cams ? lab.qc[bm + tid] : 0;
    }
    __syncthreads();
    auto flush = [&]() {
        __syncthreads();
        const unsigned n0 = s_hist[0][tid], n1 = s_hist[1][tid];
        if (n0) atomicAdd(&hist_neg[tid], (unsigned long long)n0);
        if (n1) atomicAdd(&hist_pos[tid], (unsigned long long)n1);
        s_hist[0][tid] = 0;
        s_hist[1][tid] = 0;
        __syncthreads();
    };
    int64_t since = 0;
    for (int64_t bn = c0; bn < c1; bn += DM_BN) {
        f32x16 acc[2][2];
        dm_acc_zero(acc);
        dm_tile<PIPE>(t, q, g, Q, c1, D, ldq, ldg, bm, bn, smem, acc);
        // everything per element below is 32-bit: row il of the band, the column's index as the result
        // carries it, and the band row a column forms a self pair with (-1: none)
        int64_t gpj[2], gcj[2];
        float ggj[2];
        bool jok[2];
        unsigned jg[2];
        int self_il[2];
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            const int64_t j = bn + dm_lane_col(wn, nt, lane);
            jok[nt] = j < c1;
            const int64_t jr = jok[nt] ? j : c1 - 1;
            ggj[nt] = gg[jr];
            gpj[nt] = lab.gp[jr];
            gcj[nt] = cams ? lab.gc[jr] : 0;
            jg[nt] = (unsigned)(index_base + j);
            const int64_t si = self_base + j - bm;
            self_il[nt] = self_base >= 0 && si >= 0 && si < DM_BM ? (int)si : -1;
        }
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int il = dm_lane_row(wm, mt, r, lane);
                if (il >= nq) continue;
                const float qqi = s_qq[il];
                const int64_t qpi = s_qp[il], qci = s_qc[il];
#pragma unroll
                for (int nt = 0; nt < 2; nt++) {
                    if (!jok[nt]) continue;
                    const int same = gpj[nt] == qpi;
                    if (same && cams && gcj[nt] == qci) continue;  // removed (evaluate.py:46-48)
                    if (il == self_il[nt]) continue;               // the pair of a row with itself
                    const float v = dm_value(acc[mt][nt][r], qqi, ggj[nt]);
                    int b = 0;
#pragma unroll
                    for (int s = PH_BINS / 2; s > 0; s >>= 1) b += s_edges[b + s - 1] < v ? s : 0;
                    atomicAdd(&s_hist[same][b], 1u);
                    const unsigned long long key = ((unsigned long long)ph_ordered(v) << 32) | jg[nt];
                    if (key < s_key[same][il]) atomicMin(&s_key[same][il], key);
                }
            }
        if (++since == PH_FLUSH_TILES) {
            flush();
            since = 0;
        }
    }
    flush();  // its first barrier also ends the row minima
    const int cls = tid >> 7, row = tid & (DM_BM - 1);
    const unsigned long long k = s_key[cls][row];
    if (row < nq && k != PH_NOKEY) atomicMin(&(cls ? key_pos : key_neg)[bm + row], k);
}

// One thread per query: the call's minima into the caller's in/out pairs, only ever to a smaller key.
__global__ __launch_bounds__(256) void ph_finish_kernel(const unsigned long long* __restrict__ key_pos,
                                                        const unsigned long long* __restrict__ key_neg, int64_t Q,
                                                        float* __restrict__ pos_dist, int32_t* __restrict__ pos_idx,
                                                        float* __restrict__ neg_dist, int32_t* __restrict__ neg_idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    auto merge = [&](unsigned long long k, float* dist, int32_t* idx) {
        if (k == PH_NOKEY) return;
        const float v = ph_unordered((unsigned)(k >> 32));
        const int ji = (int)(unsigned)k;
        const float ov = dist[i];
        const int oi = idx[i];
        // a row without an item so far holds +inf / -1
        if (oi < 0 || v < ov || (v == ov && ji < oi)) {
            dist[i] = v;
            idx[i] = ji;
        }
    };
    merge(key_pos[i], pos_dist, pos_idx);
    merge(key_neg[i], neg_dist, neg_idx);
}

// workspace: norms | key_pos [Q] | key_neg [Q]
static bool ph_shape_ok(int64_t Q, int64_t G) { return Q >= 0 && Q < (1ll << 31) && G >= 1 && G < (1ll << 31); }
static int64_t ph_ws_bytes(int64_t Q, int64_t G) { return dm_norm_bytes(Q, G) + 2 * Q * 8; }

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int64_t reidmi_pair_stats_workspace_bytes(int64_t Q, int64_t G) {
    return ph_shape_ok(Q, G) ? ph_ws_bytes(Q, G) : -1;
}

REIDMI_API int reidmi_pair_stats_f32(const float* q, int64_t Q, int64_t ldq, const float* g, int64_t G, int64_t ldg,
                                     int64_t D, const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids,
                                     const int64_t* g_cams, const float* edges, int n_edges, int64_t index_base,
                                     int64_t self_base, uint64_t* hist_pos, uint64_t* hist_neg, float* near_pos_dist,
                                     int32_t* near_pos_idx, float* near_neg_dist, int32_t* near_neg_idx, void* ws,
                                     int64_t ws_bytes, void* stream) {
    RM_REQUIRE(ph_shape_ok(Q, G) && D >= 1, "pair_stats: bad shape (need 0 <= Q < 2^31, 1 <= G < 2^31, D >= 1)");
    RM_REQUIRE(ldq >= D && ldg >= D, "pair_stats: row pitches must be >= D");
    RM_REQUIRE(n_edges >= 1 && n_edges <= PH_MAX_EDGES, "pair_stats: need 1 <= n_edges <= 255");
    RM_REQUIRE(edges != nullptr, "pair_stats: edges (a host array) required");
    PhEdges pe;
    for (int t = 0; t < PH_BINS; t++) pe.e[t] = __builtin_inff();
    for (int t = 0; t < n_edges; t++) {
        RM_REQUIRE(edges[t] - edges[t] == 0.0f, "pair_stats: edges must be finite");
        RM_REQUIRE(t == 0 || edges[t] >= edges[t - 1], "pair_stats: edges must be non-decreasing");
        pe.e[t] = edges[t];
    }
    RM_REQUIRE(q_pids != nullptr && g_pids != nullptr, "pair_stats: q_pids and g_pids are required");
    RM_REQUIRE((q_cams != nullptr) == (g_cams != nullptr), "pair_stats: pass both camera arrays or neither");
    RM_REQUIRE(index_base >= 0 && index_base + G <= (1ll << 31) - 1,
               "pair_stats: gallery indices must fit int32 (index_base >= 0, index_base + G <= 2^31 - 1)");
    RM_REQUIRE(self_base >= -1, "pair_stats: self_base must be >= 0, or -1 for none");
    RM_REQUIRE(hist_pos != nullptr && hist_neg != nullptr && near_pos_dist != nullptr && near_pos_idx != nullptr &&
                   near_neg_dist != nullptr && near_neg_idx != nullptr,
               "pair_stats: hist_pos, hist_neg, near_pos_dist, near_pos_idx, near_neg_dist and near_neg_idx required");
    RM_REQUIRE(ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= ph_ws_bytes(Q, G),
               "pair_stats: workspace (reidmi_pair_stats_workspace_bytes, 16-byte aligned) required");
    RM_REQUIRE(q != nullptr && g != nullptr, "pair_stats: features required");
    if (Q == 0) return OK;
    // the gallery ranges: distance.h's dm_walk_plan
    const int64_t bands = (Q + DM_BM - 1) / DM_BM, tiles = (G + DM_BN - 1) / DM_BN;
    int64_t S, range_len;
    dm_walk_plan(bands, tiles, &S, &range_len);
    RM_REQUIRE(bands * S < (1ll << 31), "pair_stats: too many query bands for one launch");
    hipStream_t s = (hipStream_t)stream;
    float* qq = (float*)ws;
    float* gg = qq + Q;
    unsigned long long* key_pos = (unsigned long long*)((char*)ws + dm_norm_bytes(Q, G));
    unsigned long long* key_neg = key_pos + Q;
    RM_CHECK_HIP(hipMemsetAsync(key_pos, 0xff, (size_t)(2 * Q * 8), s));
    RM_TRY(dm_norms(q, Q, ldq, g, G, ldg, D, qq, gg, s));
    const DmLabels lab{q_pids, q_cams, g_pids, g_cams};
    const dim3 grid((unsigned)(bands * S));
    RM_BOOL_SWITCH(dm2_ok(q, ldq, g, ldg, D), PIPE,
                   hipLaunchKernelGGL(ph_tile_kernel<PIPE>, grid, dim3(256), 0, s, q, g, (const float*)qq,
                                      (const float*)gg, Q, G, D, ldq, ldg, lab, pe, range_len, index_base, self_base,
                                      (unsigned long long*)hist_pos, (unsigned long long*)hist_neg, key_pos,
                                      key_neg));
    RM_LAUNCHED();
    hipLaunchKernelGGL(ph_finish_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s,
                       (const unsigned long long*)key_pos, (const unsigned long long*)key_neg, Q, near_pos_dist,
                       near_pos_idx, near_neg_dist, near_neg_idx);
    RM_LAUNCHED();
    return OK;
}
