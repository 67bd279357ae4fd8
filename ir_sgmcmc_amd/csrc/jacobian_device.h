// det J of a transformation in [-1,1] at one voxel: GradientOperator(transformation=True) + calc_det_J
// (utils/diff_op.py:78-96, utils/util.py:72-91).  The one place this arithmetic lives: the per-sample fold count
// (data_kernels.hip: log_det_kernel) and the Jacobian posterior (jacobian_kernels.hip) call it, so they cannot disagree about det.
#pragma once
#include "common.h"

namespace irs {

__device__ __forceinline__ float fwd_diff(const float* __restrict__ f, int64_t p, int pos, int n, int64_t stride) {
    return pos + 1 < n ? f[p + stride] - f[p] : f[p] - f[p - stride];  // replicated last difference
}

// t: the three channels (x, y, z components, vol.V apart) of one chain; p = (z H + y) W + x.  Forward differences with the last
// one replicated, divided by the normalised spacing 2 / (N - 1), then the six products in the order of utils/util.py:84-89.
// Every dim must be >= 2 (the replicated difference reads the voxel before the last).
__device__ __forceinline__ float det_jacobian(const float* __restrict__ t, int64_t p, int x, int y, int z, const Vol& vol) {
    const int64_t plane = (int64_t)vol.W * vol.H;
    const float sp[3] = {2.0f / (float)(vol.W - 1), 2.0f / (float)(vol.H - 1), 2.0f / (float)(vol.D - 1)};
    float n[3][3];  // n[a][comp]
#pragma unroll
    for (int comp = 0; comp < 3; ++comp) {
        const float* f = t + comp * vol.V;
        n[0][comp] = fwd_diff(f, p, x, vol.W, 1) / sp[0];
        n[1][comp] = fwd_diff(f, p, y, vol.H, vol.W) / sp[1];
        n[2][comp] = fwd_diff(f, p, z, vol.D, plane) / sp[2];
    }
    // nabla_x = n[.][0], nabla_y = n[.][1], nabla_z = n[.][2]; formula of utils/util.py:84-89
    return n[0][0] * n[1][1] * n[2][2] + n[0][1] * n[1][2] * n[2][0] + n[0][2] * n[1][0] * n[2][1] -
           n[2][0] * n[1][1] * n[0][2] - n[2][1] * n[1][2] * n[0][0] - n[2][2] * n[1][0] * n[0][1];
}

}  // namespace irs
