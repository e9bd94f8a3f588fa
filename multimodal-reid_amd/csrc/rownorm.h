// rownorm.h — the arithmetic of F.normalize(x, p=2, dim=1) (reidmi_l2norm_f32), one definition for
// every kernel that normalises a row: distance.hip's row_sqnorm_kernel / row_scale_kernel and
// combine.hip's fused normalise.  Bit-exact contract: the squared norm is ONE fmaf chain over the
// columns ascending, from +0; the row is divided (correctly rounded) by max(sqrt(ss), 1e-12).
#pragma once
#include "common.h"

namespace reidmi {

// One link of the squared-norm chain: acc + v * v, fused.
__device__ __forceinline__ float l2_sq_step(float acc, float v) { return __builtin_fmaf(v, v, acc); }

// The divisor of a row whose squared norm is ss.
__device__ __forceinline__ float l2_denominator(float ss) {
    const float nrm = __builtin_sqrtf(ss);
    return nrm < 1e-12f ? 1e-12f : nrm;
}

__device__ __forceinline__ float l2_scale(float v, float den) { return v / den; }

}  // namespace reidmi
