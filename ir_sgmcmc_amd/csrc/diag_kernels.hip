// Split-R-hat of the displacement over chains (absent in the reference; Gelman et al., BDA3 section 11.4).
//
//  - moment update: one stream over the (C,3,D,H,W) sample and the (mean, m2) of one half, all chains in one launch.  The
//    three arrays are flat; 16-byte accesses when all three base pointers allow them (the half-1 slice of a state whose
//    C*3*D*H*W is not a multiple of 4 does not), a scalar tail for the last n % 4 elements.  Grid-stride over a capped grid.
//  - finalize: one voxel per thread reads the 2C means and M2 of its three components, writes max over the components of
//    R-hat, and accumulates the masked summary in registers; block partials go to the workspace and one block reduces them
//    in fixed order.  The grid depends on the volume only, so two calls are bit-identical.
#include <algorithm>

#include "kernels.h"

namespace irs {
namespace {

constexpr int kDiagMaxBlocks = 2048;  // 256 CUs x 8 blocks of 4 wavefronts: one full wave of resident blocks
constexpr float kDiagInf = __builtin_huge_valf();

__device__ __forceinline__ void welford(float x, float& mean, float& m2, float k) {
    const float delta = x - mean;
    mean += delta / k;
    m2 += delta * (x - mean);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void chain_moments_kernel(const float* __restrict__ x, float* __restrict__ mean,
                                                              float* __restrict__ m2, int64_t n, float k) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t done = 0;
    if (VEC) {
        const int64_t n4 = n >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(x);
        float4* mu4 = reinterpret_cast<float4*>(mean);
        float4* m24 = reinterpret_cast<float4*>(m2);
        for (int64_t i = tid; i < n4; i += stride) {
            const float4 v = x4[i];
            float4 mu = mu4[i], s = m24[i];
            welford(v.x, mu.x, s.x, k);
            welford(v.y, mu.y, s.y, k);
            welford(v.z, mu.z, s.z, k);
            welford(v.w, mu.w, s.w, k);
            mu4[i] = mu;
            m24[i] = s;
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += stride) {
        float mu = mean[i], s = m2[i];
        welford(x[i], mu, s, k);
        mean[i] = mu;
        m2[i] = s;
    }
}

// split-R-hat of one component from the M = 2C sequences of n samples: W = mean of M2_m / (n - 1), B / n = variance of the
// sequence means, var+ = (n - 1) / n W + B / n, R-hat = sqrt(var+ / W).  Never NaN.
__device__ __forceinline__ float rhat_component(const float* __restrict__ mean, const float* __restrict__ m2, int64_t seq_stride,
                                                int M, double n) {
    // one pass: the means shifted by the first one (differences of two floats are exact in double), so sum d^2 - (sum d)^2 / M
    // cancels only as far as the means really are equal
    const float ref = mean[0];
    double sd = 0.0, sdd = 0.0, w = 0.0;
    for (int m = 0; m < M; ++m) {
        const double d = (double)mean[m * seq_stride] - (double)ref;
        sd += d;
        sdd += d * d;
        w += (double)m2[m * seq_stride];
    }
    w /= (double)M * (n - 1.0);
    double b = (sdd - sd * sd / M) / (M - 1);  // B / n; M = 2C >= 2
    if (b < 0.0) b = 0.0;                      // rounding; a NaN stays and ends as inf below
    if (!(w > 0.0)) return b == 0.0 ? 1.0f : kDiagInf;  // W = 0 (or not finite): equal sequences give 1, anything else inf
    const double r = sqrt(((n - 1.0) / n * w + b) / w);
    return r == r ? (float)r : kDiagInf;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, kWave));
    return v;
}

// summary partials, 5 doubles per block: voxels, above thr0, above thr1, max, sum (result valid in thread 0)
__device__ __forceinline__ void block_summary(double (&acc)[5], double* smem) {
    double s[4] = {acc[0], acc[1], acc[2], acc[4]};
    block_sum<4>(s, smem);
    __syncthreads();  // block_sum's thread 0 reads smem after its barrier; the max below reuses it
    double mx = wave_max(acc[3]);
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    if (lane == 0) smem[wid] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; ++w) mx = fmax(mx, smem[w]);
        acc[0] = s[0];
        acc[1] = s[1];
        acc[2] = s[2];
        acc[3] = mx;
        acc[4] = s[3];
    }
}

__global__ __launch_bounds__(kBlock) void split_rhat_kernel(const float* __restrict__ mean, const float* __restrict__ m2, int C,
                                                            float n, const uint8_t* __restrict__ mask, float thr0, float thr1,
                                                            float* __restrict__ rhat, double* __restrict__ partials, int64_t V) {
    __shared__ double smem[4 * (kBlock / kWave)];
    const int M = 2 * C;
    const int64_t seq = 3 * V;  // sequence m = half * C + chain starts at m * 3V; component j at + j * V
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        float r = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) r = fmaxf(r, rhat_component(mean + j * V + v, m2 + j * V + v, seq, M, (double)n));
        rhat[v] = r;
        if (!mask || mask[v]) {
            acc[0] += 1.0;
            acc[1] += r > thr0 ? 1.0 : 0.0;
            acc[2] += r > thr1 ? 1.0 : 0.0;
            acc[3] = fmax(acc[3], (double)r);
            acc[4] += (double)r;
        }
    }
    block_summary(acc, smem);
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < 5; ++i) partials[(int64_t)blockIdx.x * 5 + i] = acc[i];
}

// one block: the per-block partials in fixed order
__global__ __launch_bounds__(kBlock) void split_rhat_reduce_kernel(const double* __restrict__ partials, int nblocks,
                                                                   double* __restrict__ summary) {
    __shared__ double smem[4 * (kBlock / kWave)];
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += kBlock) {
        acc[0] += partials[b * 5 + 0];
        acc[1] += partials[b * 5 + 1];
        acc[2] += partials[b * 5 + 2];
        acc[3] = fmax(acc[3], partials[b * 5 + 3]);
        acc[4] += partials[b * 5 + 4];
    }
    block_summary(acc, smem);
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < 5; ++i) summary[i] = acc[i];
}

}  // namespace

int split_rhat_blocks(int64_t V) { return (int)std::min<int64_t>((V + kBlock - 1) / kBlock, kDiagMaxBlocks); }

void launch_chain_moments(const float* x, float* mean, float* m2, int64_t n, int k, hipStream_t st) {
    const bool vec = (((uintptr_t)x | (uintptr_t)mean | (uintptr_t)m2) & 15) == 0;
    const int64_t units = vec ? (n + 3) / 4 : n;
    const dim3 grid((unsigned)std::min<int64_t>((units + kBlock - 1) / kBlock, kDiagMaxBlocks));
    if (vec) hipLaunchKernelGGL(chain_moments_kernel<true>, grid, dim3(kBlock), 0, st, x, mean, m2, n, (float)k);
    else hipLaunchKernelGGL(chain_moments_kernel<false>, grid, dim3(kBlock), 0, st, x, mean, m2, n, (float)k);
}

void launch_split_rhat(const float* mean, const float* m2, int C, int n, const uint8_t* mask, float thr0, float thr1, float* rhat,
                       double* summary, double* partials, int64_t V, hipStream_t st) {
    const int blocks = split_rhat_blocks(V);
    hipLaunchKernelGGL(split_rhat_kernel, dim3(blocks), dim3(kBlock), 0, st, mean, m2, C, (float)n, mask, thr0, thr1, rhat,
                       partials, V);
    hipLaunchKernelGGL(split_rhat_reduce_kernel, dim3(1), dim3(kBlock), 0, st, partials, blocks, summary);
}

}  // namespace irs
