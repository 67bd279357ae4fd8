// The bin rule and the LDS histogram add the histogram kernels share (similarity_kernels.hip, residual_kernels.hip,
// mask_kernels.hip).
#pragma once
#include "common.h"

namespace irs {

// The bin rule, in fp32 with every operation rounded once: t = (x - lo) * inv_w -- a difference, then a product: nothing to
// contract -- and b = min(last, max(0, floor(t))) with last = bins - 1 as a float.  Clamped as floats: floor(t) of a finite
// value far outside the range need not fit an int.
__device__ __forceinline__ int hist_bin(float x, float lo, float inv_w, float last) {
    return (int)fminf(fmaxf(floorf(__fmul_rn(__fsub_rn(x, lo), inv_w)), 0.0f), last);
}

// h[cell] += 1 for every lane with take set.  Wave-uniform control flow: every lane of the wavefront calls it.  One LDS
// address hit by all 64 lanes serialises (a constant region: background, saturation): with `aggregate`, when every voxel the
// wavefront adds in this step falls into ONE cell, its first taking lane adds their number instead -- two ballots and a
// v_readlane, still one LDS instruction per step.
__device__ __forceinline__ void hist_add(uint32_t* h, bool take, int cell, bool aggregate) {
    if (aggregate) {
        const unsigned long long todo = __ballot(take);
        if (todo == 0) return;
        const int leader = __ffsll(todo) - 1;
        const int cl = __builtin_amdgcn_readlane(cell, leader);
        if (__ballot(take && cell != cl) == 0) {  // one bin for the whole wavefront: one add of their number
            if ((int)(threadIdx.x & (kWave - 1)) == leader) atomicAdd(&h[cl], (uint32_t)__popcll(todo));
            return;
        }
    }
    if (take) atomicAdd(&h[cell], 1u);
}

}  // namespace irs
