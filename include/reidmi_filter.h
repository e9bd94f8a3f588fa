/*
 * reidmi_filter.h — the filter argument of reidmi_search_filtered_f32 and
 * reidmi_search_prefiltered_filtered_f32 (reidmi.h, which includes this file and states the
 * clauses).  A host struct of DEVICE pointers; a clause whose pointers are all NULL is absent.
 * It is a header of its own so that the structs reidmi.h itself defines stay the model's weight
 * and source structs; the ctypes binding reads it like reidmi.h (multimodal-reid_amd/_lib.py).
 */
#ifndef REIDMI_FILTER_H
#define REIDMI_FILTER_H
#include <stdint.h>

typedef struct reidmi_search_filter {
    const uint8_t* g_valid;
    const int64_t* g_cam;
    const int64_t* q_cam_mask;
    const int64_t* g_time;
    const int64_t* q_time_lo;
    const int64_t* q_time_hi;
    const int64_t* g_group;
    const int64_t* q_group;
} reidmi_search_filter;

#endif
