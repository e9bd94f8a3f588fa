// cluster.h — what both DBSCAN sources need (internal, not part of the C ABI):
//   cluster.hip          reidmi_dbscan_f32: the passes over the fp32 distance tiles, and the O(N)
//                        kernels between and after the passes of either source
//   rerank_jaccard.hip   reidmi_dbscan_jaccard: the passes over the sparse self-Jaccard rows
// Here: the lock-free find / union on parent[] (cluster.hip's head says why their result does not
// depend on scheduling), the O(N) state both calls keep in their workspace, and the launchers of
// the O(N) kernels.  A pass is whatever fills counts, joins parent[] and lowers border[].
#pragma once
#include "common.h"

namespace reidmi {

constexpr int DBS_NONE = 0x7fffffff;  // border root of a row without a core neighbour
enum DbsPass : int { DBS_COUNT = 0, DBS_UNION = 1, DBS_BORDER = 2 };

__device__ __forceinline__ int dbs_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int dbs_find(const int32_t* parent, int a) {
    for (;;) {
        const int p = dbs_load(parent + a);  // p <= a: the walk ends
        if (p == a) return a;
        a = p;
    }
}

// Joins the trees of a and b; returns the joined tree's root as far as this thread saw it.
__device__ __forceinline__ int dbs_union(int32_t* parent, int a, int b) {
    for (;;) {
        a = dbs_find(parent, a);
        b = dbs_find(parent, b);
        if (a == b) return a;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return lo;
        a = old;  // hi was hooked meanwhile, under old < hi
        b = lo;
    }
}

// The O(N) state of a run, as byte offsets from a 16-byte aligned base: parent | border | number |
// block sums (nb of them).  False for N outside [1, 2^31).
struct DbsState {
    int64_t parent_off, border_off, number_off, bsum_off, nb, bytes;
};
bool dbs_state(int64_t N, DbsState* w);

// cluster.hip
// core = counts >= min_samples, parent = itself, border = DBS_NONE
int dbs_init_launch(const int32_t* counts, int64_t N, int min_samples, uint8_t* core, int32_t* parent, int32_t* border,
                    hipStream_t s);
// every parent becomes its root (after the union pass)
int dbs_compress_launch(int32_t* parent, int64_t N, hipStream_t s);
// cluster numbers by lowest core index (number, bsum: scratch), n_clusters and the labels
int dbs_labels_launch(const uint8_t* core, const int32_t* parent, const int32_t* border, int32_t* number, int32_t* bsum,
                      int64_t nb, int64_t N, int32_t* n_clusters, int32_t* labels, hipStream_t s);

}  // namespace reidmi
