// gemm_prof.hip — live GEMM timing (host code only): the event records behind reidmi_prof_*.
// bench.py measures the roofline of the dominant kernel with HIP events recorded on the
// launch stream around each GEMM of the timed region (reidmi_prof_*).  Off by default.
// gemm_f16 (gemm.hip) brackets its launch with prof_begin / prof_end (gemm.h).
#include "gemm.h"

#include <mutex>
#include <vector>

namespace reidmi {

namespace prof {
struct Rec {
    hipEvent_t a, b;
    double flops;
    int epi;
};
static bool enabled = false;
static std::mutex mu;
static std::vector<Rec> recs;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
static size_t used = 0;
}  // namespace prof

int prof_begin(double flops, int epi, hipStream_t s, hipEvent_t* end) {
    *end = nullptr;
    if (!prof::enabled) return OK;
    std::lock_guard<std::mutex> g(prof::mu);
    if (prof::used == prof::pool.size()) {
        hipEvent_t a, b;
        RM_CHECK_HIP(hipEventCreate(&a));
        RM_CHECK_HIP(hipEventCreate(&b));
        prof::pool.push_back({a, b});
    }
    auto pr = prof::pool[prof::used++];
    prof::recs.push_back({pr.first, pr.second, flops, epi});
    RM_CHECK_HIP(hipEventRecord(pr.first, s));
    *end = pr.second;
    return OK;
}

int prof_end(hipEvent_t end, hipStream_t s) {
    RM_CHECK_HIP(hipEventRecord(end, s));
    return OK;
}

}  // namespace reidmi

using namespace reidmi;

REIDMI_API int reidmi_prof_enable(int on) {
    std::lock_guard<std::mutex> g(prof::mu);
    prof::enabled = on != 0;
    prof::recs.clear();
    prof::used = 0;
    return OK;
}

// Sum of device time (ms), launch count and algorithmic FLOPs of the recorded GEMM launches
// with epilogue `epi` (-1: all) and at least `min_flops` each.  Waits for the recorded
// events; then clears the record.
REIDMI_API int reidmi_prof_collect_min(int epi, double min_flops, double* total_ms, int64_t* count, double* flops) {
    std::lock_guard<std::mutex> g(prof::mu);
    double t = 0, f = 0;
    int64_t n = 0;
    for (auto& r : prof::recs) {
        if (epi >= 0 && r.epi != epi) continue;
        if (r.flops < min_flops) continue;
        RM_CHECK_HIP(hipEventSynchronize(r.b));
        float ms = 0;
        RM_CHECK_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        t += ms;
        f += r.flops;
        n++;
    }
    if (total_ms) *total_ms = t;
    if (count) *count = n;
    if (flops) *flops = f;
    prof::recs.clear();
    prof::used = 0;
    return OK;
}

REIDMI_API int reidmi_prof_collect(int epi, double* total_ms, int64_t* count, double* flops) {
    return reidmi_prof_collect_min(epi, 0.0, total_ms, count, flops);
}
