// Device helpers of the label counts, shared by label_kernels.hip (irs_label_posterior_update) and native_posterior_kernels.hip
// (irs_native_posterior_update): which structure a label value is, and the per-wavefront count behind the per-record volumes.
#pragma once
#include "kernels.h"

namespace irs {

__device__ __forceinline__ int structure_of(int x, const SurfLabels& lab, int K) {
    int idx = -1;  // labels are distinct: at most one matches
    for (int j = 0; j < K; ++j) idx = lab.v[j] == x ? j : idx;
    return idx;
}

// cnt[j] += number of lanes holding j, for every j >= 0 held in the wavefront: one LDS add per distinct value (a single
// address hit by all 64 lanes would serialise).  Every lane of the wavefront must reach the call (ballot + shuffle): a lane
// with nothing to count passes j = -1
__device__ __forceinline__ void wave_count(int j, int* cnt) {
    unsigned long long todo = __ballot(j >= 0);
    const int lane = threadIdx.x & (kWave - 1);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int jl = __shfl(j, leader, kWave);
        const unsigned long long m = __ballot(j == jl);
        if (lane == leader) atomicAdd(&cnt[jl], __popcll(m));
        todo &= ~m;
    }
}

}  // namespace irs
