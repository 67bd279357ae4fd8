// The contour predicate the surface kernels share (metric_kernels.hip pass W, surface_kernels.hip).
#pragma once
#include "common.h"

namespace irs {

// sitk.LabelContour with face connectivity: a voxel of `lab` with an in-volume face neighbour that is not `lab`
__device__ __forceinline__ bool on_contour(const int16_t* __restrict__ s, int z, int y, int x, int lab, const Vol& vol) {
    const int64_t HW = (int64_t)vol.H * vol.W;
    const int64_t i = z * HW + (int64_t)y * vol.W + x;
    if (s[i] != lab) return false;
    return (x > 0 && s[i - 1] != lab) || (x + 1 < vol.W && s[i + 1] != lab) || (y > 0 && s[i - vol.W] != lab) ||
           (y + 1 < vol.H && s[i + vol.W] != lab) || (z > 0 && s[i - HW] != lab) || (z + 1 < vol.D && s[i + HW] != lab);
}

}  // namespace irs
