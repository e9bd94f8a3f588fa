// capi.hip — error state and version of the libreidmi C ABI (include/reidmi.h).
#include "common.h"

namespace reidmi {
static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
int fail(int code, const std::string& m) {
    g_err = m;
    return code;
}
}  // namespace reidmi

REIDMI_API const char* reidmi_last_error(void) { return reidmi::g_err.c_str(); }
// 2: per-call GEMM tiling / distance variant entry points replace the process-global setters;
// 3: RCCL exchange (reidmi_comm_*); re-ranking without capacity limits;
// 4: the forced-variant entry points moved to libreidmi_tools.so (include/reidmi_tools.h);
//    weight packing (reidmi_vit_weights_pack / reidmi_text_weights_pack);
// 5: re-ranked rank lists (reidmi_rr_jaccard_topk_rows);
// 6: merged rank lists (reidmi_search_merge_f32);
// 7: combined feature rows (reidmi_combine_rows_f32);
// 8: matrix-free evaluation (reidmi_eval_feat_f32, reidmi_evf_*);
// 9: bounded search (reidmi_search_bounded_f32);
// 10: clustering (reidmi_dbscan_f32);
// 11: clustering on the k-reciprocal Jaccard distance (reidmi_rr_jaccard_self_rows,
//     reidmi_dbscan_jaccard);
// 12: pair statistics (reidmi_pair_stats_f32);
// 13: pre-filtered search (reidmi_search_prefiltered_f32, reidmi_search_prefilter_applies,
//     reidmi_search_prefiltered_workspace_bytes).
REIDMI_API int reidmi_abi_version(void) { return 14; }
