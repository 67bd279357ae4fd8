// Per-voxel arithmetic of the displacement credible intervals: the bin a record's displacement counts
// into, and the histogram quantile.  Plain host / device functions over scalars, so every kernel computes the same thing.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace irs {

// float32: one subtraction, one product, floor; then the clamp (a NaN lands on -B, hence in bin 0) and, in integers, the
// offset.  The subtraction and the product are two separately rounded operations: there is no multiply-add to contract.
__host__ __device__ inline int quantile_bin(float x, float centre, float inv_width, int B) {
#ifdef __HIP_DEVICE_COMPILE__
    float t = floorf(__fmul_rn(__fsub_rn(x, centre), inv_width));
#else
    volatile float d = x - centre;
    float t = floorf(d * inv_width);
#endif
    t = fminf(fmaxf(t, -(float)B), (float)B);
    const int b = (int)t + B / 2;
    return b < 0 ? 0 : b > B - 1 ? B - 1 : b;
}

// the quantile whose rank r = p n falls into bin b (cum_prev < r <= cum_prev + count): linear within the bin, in double;
// NaN (out of range) in the two open-ended bins
__host__ __device__ inline float quantile_value(double centre, int b, int B, double r, int cum_prev, int count, double width,
                                                double scale) {
    if (b == 0 || b == B - 1) return __builtin_nanf("");
    return (float)(scale * (centre + ((double)(b - B / 2) + (r - (double)cum_prev) / (double)count) * width));
}

}  // namespace irs
