// admit.h — which gallery items a query may match at all: the one definition of the search side's
// admissibility (reidmi_search_f32 and everything built on it).  Item j is admitted for query i iff
// every clause that is present holds:
//
//   label rule   not (g_pids[j] == q_pids[i] and g_cams[j] == q_cams[i])          evaluate.py:46-48
//   valid        g_valid[j] != 0
//   camera mask  0 <= g_cam[j] < 64 and bit g_cam[j] of q_cam_mask[i] is set
//   time window  q_time_lo[i] <= g_time[j] <= q_time_hi[i]
//   group        g_group[j] != q_group[i]
//
// search_f32_kernel's epilogue (search.hip), sp_threshold_kernel and sp_select_kernel
// (search_prefilter.hip) call sr_admit and nothing else decides.  The evaluator, the pair statistics
// and DBSCAN keep their own use of the label rule (DmLabels, distance.h).
#pragma once
#include <type_traits>

#include "common.h"

namespace reidmi {

// Device pointers; a null gallery-side pointer says that the clause is absent (sr_filter_make has
// refused the half-given ones).  The label arrays are all present or all null.
struct SrFilter {
    static constexpr bool kClauses = true;
    const int64_t *qp, *qc, *gp, *gc;
    const uint8_t* g_valid;
    const int64_t *g_cam, *q_cam_mask;
    const int64_t *g_time, *q_time_lo, *q_time_hi;
    const int64_t *g_group, *q_group;
};
// The label arrays alone: what search_f32_kernel's instantiations without a filter take, so that
// their kernel arguments, and with them their code, are those of the search before filters.
struct SrLabels {
    static constexpr bool kClauses = false;
    const int64_t *qp, *qc, *gp, *gc;
};

// The query side of one row and the gallery side of one item: what the present clauses read, the
// rest zero.  `labels` / `clauses` say which halves the caller wants read at all (compile-time
// constants in search_f32_kernel, where an absent half costs nothing).
struct SrRow {
    int64_t pid, cam, mask, t_lo, t_hi, group;
};
// SrRow with the labels left where they are (search_f32_kernel's LDS copies): read at the compare.
struct SrRowRef {
    const int64_t &pid, &cam;
    int64_t mask, t_lo, t_hi, group;
};
struct SrItem {
    int64_t pid, cam, fcam, time, group;
    bool valid;
};

// The valid clause alone: the cheapest one, a whole column's test.
__device__ __forceinline__ bool sr_item_valid(const SrFilter& f, int64_t j) {
    return f.g_valid == nullptr || f.g_valid[j] != 0;
}

template <class F>
__device__ __forceinline__ void sr_row_labels(const F& f, int64_t i, SrRow& r) {
    r.pid = f.qp[i];
    r.cam = f.qc[i];
}
template <class R>
__device__ __forceinline__ void sr_row_clauses(const SrFilter& f, int64_t i, R& r) {
    r.mask = f.g_cam != nullptr ? f.q_cam_mask[i] : 0;
    r.t_lo = f.g_time != nullptr ? f.q_time_lo[i] : 0;
    r.t_hi = f.g_time != nullptr ? f.q_time_hi[i] : 0;
    r.group = f.g_group != nullptr ? f.q_group[i] : 0;
}
__device__ __forceinline__ SrRow sr_row(const SrFilter& f, bool labels, bool clauses, int64_t i) {
    SrRow r = {0, 0, 0, 0, 0, 0};
    if (labels) sr_row_labels(f, i, r);
    if (clauses) sr_row_clauses(f, i, r);
    return r;
}

template <class F>
__device__ __forceinline__ SrItem sr_item(const F& f, bool labels, bool clauses, int64_t j) {
    SrItem g = {0, 0, 0, 0, 0, true};
    if (labels) {
        g.pid = f.gp[j];
        g.cam = f.gc[j];
    }
    if constexpr (F::kClauses) {
        if (clauses) {
            g.valid = sr_item_valid(f, j);
            if (f.g_cam != nullptr) g.fcam = f.g_cam[j];
            if (f.g_time != nullptr) g.time = f.g_time[j];
            if (f.g_group != nullptr) g.group = f.g_group[j];
        }
    }
    return g;
}

// THE rule.  The clauses are independent tests joined by "and": their order cannot show.
template <class F, class R>
__device__ __forceinline__ bool sr_admit(const F& f, bool labels, bool clauses, const R& r, const SrItem& g) {
    if (labels && g.pid == r.pid && g.cam == r.cam) return false;  // evaluate.py:46-48
    if constexpr (F::kClauses) {
        if (clauses) {
            if (!g.valid) return false;
            if (f.g_cam != nullptr && !((uint64_t)g.fcam < 64 && (((uint64_t)r.mask >> (g.fcam & 63)) & 1) != 0))
                return false;
            if (f.g_time != nullptr && !(r.t_lo <= g.time && g.time <= r.t_hi)) return false;
            if (f.g_group != nullptr && g.group == r.group) return false;
        }
    }
    return true;
}

__host__ __device__ inline bool sr_has_clauses(const SrFilter& f) {
    return f.g_valid != nullptr || f.g_cam != nullptr || f.g_time != nullptr || f.g_group != nullptr;
}

// The entry points' four label pointers and their reidmi_search_filter (nullable) as one SrFilter;
// a half-given clause is refused by name.  Host code, before any HIP call.
inline int sr_filter_make(const int64_t* q_pids, const int64_t* q_cams, const int64_t* g_pids, const int64_t* g_cams,
                          const reidmi_search_filter* flt, SrFilter* out) {
    const int nlab = (q_pids != nullptr) + (q_cams != nullptr) + (g_pids != nullptr) + (g_cams != nullptr);
    RM_REQUIRE(nlab == 0 || nlab == 4, "search: pass all four label arrays or none");
    *out = SrFilter{q_pids, q_cams, g_pids, g_cams, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (flt == nullptr) return OK;
    RM_REQUIRE((flt->g_cam != nullptr) == (flt->q_cam_mask != nullptr),
               "search: filter clause `camera mask` is half given: pass g_cam and q_cam_mask together");
    const int ntime = (flt->g_time != nullptr) + (flt->q_time_lo != nullptr) + (flt->q_time_hi != nullptr);
    RM_REQUIRE(ntime == 0 || ntime == 3,
               "search: filter clause `time window` is half given: pass g_time, q_time_lo and q_time_hi together");
    RM_REQUIRE((flt->g_group != nullptr) == (flt->q_group != nullptr),
               "search: filter clause `group` is half given: pass g_group and q_group together");
    out->g_valid = flt->g_valid;
    out->g_cam = flt->g_cam;
    out->q_cam_mask = flt->q_cam_mask;
    out->g_time = flt->g_time;
    out->q_time_lo = flt->q_time_lo;
    out->q_time_hi = flt->q_time_hi;
    out->g_group = flt->g_group;
    out->q_group = flt->q_group;
    return OK;
}

}  // namespace reidmi
