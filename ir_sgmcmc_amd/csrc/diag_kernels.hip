// Split-R-hat, split effective sample size and MCSE of the displacement over chains (absent in the reference; Gelman et al.,
// BDA3 sections 11.4 and 11.5).
//
//  - moment update: one stream over the (C,3,D,H,W) sample and the (mean, m2) of one half, all chains in one launch.  The
//    three arrays are flat; 16-byte accesses when all three base pointers allow them (the half-1 slice of a state whose
//    C*3*D*H*W is not a multiple of 4 does not), a scalar tail for the last n % 4 elements.  Grid-stride over a capped grid.
//  - finalize: one voxel per thread reads the 2C means and M2 of its three components, writes max over the components of
//    R-hat, and accumulates the masked summary in registers; block partials go to the workspace and one block reduces them
//    in fixed order.  The grid depends on the volume only, so two calls are bit-identical.
//  - variogram update: the same flat stream over the (C,3,D,H,W) sample, plus the ring of the last L samples (L,C,3,D,H,W)
//    and the lag sums (L,3,D,H,W).  Each element's C chain values stay in registers while its lags are read; the chains are
//    summed in fixed order, and the sample goes into the ring after every lag is read (lag L lives in its slot).
//  - ESS finalize: one voxel per thread, var+ from the moments as R-hat has it, the variogram scan as far as BDA3's
//    truncation rule needs, and the same fixed-order partials as the R-hat finalize.
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

// W and B / n of one component from the M = 2C sequences of n samples: W = mean of M2_m / (n - 1), B / n = variance of the
// sequence means.  B / n >= 0 unless it is NaN.  Shared by R-hat and ESS.
__device__ __forceinline__ void split_within_between(const float* __restrict__ mean, const float* __restrict__ m2,
                                                     int64_t seq_stride, int M, double n, double& w, double& b) {
    // one pass: the means shifted by the first one (differences of two floats are exact in double), so sum d^2 - (sum d)^2 / M
    // cancels only as far as the means really are equal
    const float ref = mean[0];
    double sd = 0.0, sdd = 0.0;
    w = 0.0;
    for (int m = 0; m < M; ++m) {
        const double d = (double)mean[m * seq_stride] - (double)ref;
        sd += d;
        sdd += d * d;
        w += (double)m2[m * seq_stride];
    }
    w /= (double)M * (n - 1.0);
    b = (sdd - sd * sd / M) / (M - 1);  // B / n; M = 2C >= 2
    if (b < 0.0) b = 0.0;               // rounding; a NaN stays
}

// split-R-hat of one component: var+ = (n - 1) / n W + B / n, R-hat = sqrt(var+ / W).  Never NaN.
__device__ __forceinline__ float rhat_component(const float* __restrict__ mean, const float* __restrict__ m2, int64_t seq_stride,
                                                int M, double n) {
    double w, b;
    split_within_between(mean, m2, seq_stride, M, n, w, b);  // a NaN B ends as inf below
    if (!(w > 0.0)) return b == 0.0 ? 1.0f : kDiagInf;  // W = 0 (or not finite): equal sequences give 1, anything else inf
    const double r = sqrt(((n - 1.0) / n * w + b) / w);
    return r == r ? (float)r : kDiagInf;
}

// MIN: slot 3 of the summary is a minimum (ESS) rather than a maximum (R-hat)
template <bool MIN>
__device__ __forceinline__ double extremum(double a, double b) {
    return MIN ? fmin(a, b) : fmax(a, b);
}

template <bool MIN>
__device__ __forceinline__ double wave_extremum(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = extremum<MIN>(v, __shfl_down(v, off, kWave));
    return v;
}

// summary partials, 5 doubles per block: three counts, the extremum, a sum (result valid in thread 0)
template <bool MIN = false>
__device__ __forceinline__ void block_summary(double (&acc)[5], double* smem) {
    double s[4] = {acc[0], acc[1], acc[2], acc[4]};
    block_sum<4>(s, smem);
    __syncthreads();  // block_sum's thread 0 reads smem after its barrier; the extremum below reuses it
    double mx = wave_extremum<MIN>(acc[3]);
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    if (lane == 0) smem[wid] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; ++w) mx = extremum<MIN>(mx, smem[w]);
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
template <bool MIN>
__global__ __launch_bounds__(kBlock) void split_summary_reduce_kernel(const double* __restrict__ partials, int nblocks,
                                                                      double* __restrict__ summary) {
    __shared__ double smem[4 * (kBlock / kWave)];
    double acc[5] = {0.0, 0.0, 0.0, MIN ? (double)kDiagInf : 0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += kBlock) {
        acc[0] += partials[b * 5 + 0];
        acc[1] += partials[b * 5 + 1];
        acc[2] += partials[b * 5 + 2];
        acc[3] = extremum<MIN>(acc[3], partials[b * 5 + 3]);
        acc[4] += partials[b * 5 + 4];
    }
    block_summary<MIN>(acc, smem);
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < 5; ++i) summary[i] = acc[i];
}

// ---- split ESS (BDA3 section 11.5)

constexpr int kMaxChains = 8;  // IRS_MAX_CHAINS: each chain's value of an element stays in registers across the lags

__device__ __forceinline__ float sq(float d) { return d * d; }

// x (C,E), ring (L,C,E), vsum (L,E) flat; lags = min(k - 1, L) lags to add, slot = (k - 1) mod L, where x goes
template <bool VEC>
__global__ __launch_bounds__(kBlock) void chain_variogram_kernel(const float* __restrict__ x, float* __restrict__ ring,
                                                                 float* __restrict__ vsum, int C, int64_t E, int L, int lags,
                                                                 int slot) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t CE = (int64_t)C * E;
    int64_t done = 0;
    if (VEC) {  // E % 4 == 0: every chain's and every slot's base is 16-byte aligned
        const int64_t E4 = E >> 2;
        for (int64_t i = tid; i < E4; i += stride) {
            float4 xv[kMaxChains];
#pragma unroll
            for (int c = 0; c < kMaxChains; ++c)
                if (c < C) xv[c] = reinterpret_cast<const float4*>(x + c * E)[i];
            for (int t = 1; t <= lags; ++t) {
                const int s = slot - t < 0 ? slot - t + L : slot - t;
                const float* r = ring + s * CE;
                float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int c = 0; c < kMaxChains; ++c)
                    if (c < C) {
                        const float4 rv = reinterpret_cast<const float4*>(r + c * E)[i];
                        d.x += sq(xv[c].x - rv.x);
                        d.y += sq(xv[c].y - rv.y);
                        d.z += sq(xv[c].z - rv.z);
                        d.w += sq(xv[c].w - rv.w);
                    }
                float4* vs = reinterpret_cast<float4*>(vsum + (t - 1) * E);
                float4 acc = vs[i];
                acc.x += d.x;
                acc.y += d.y;
                acc.z += d.z;
                acc.w += d.w;
                vs[i] = acc;
            }
            float* w = ring + slot * CE;
#pragma unroll
            for (int c = 0; c < kMaxChains; ++c)
                if (c < C) reinterpret_cast<float4*>(w + c * E)[i] = xv[c];
        }
        done = E4 << 2;
    }
    for (int64_t i = done + tid; i < E; i += stride) {
        float xv[kMaxChains];
#pragma unroll
        for (int c = 0; c < kMaxChains; ++c)
            if (c < C) xv[c] = x[c * E + i];
        for (int t = 1; t <= lags; ++t) {
            const int s = slot - t < 0 ? slot - t + L : slot - t;
            const float* r = ring + s * CE;
            float d = 0.0f;
#pragma unroll
            for (int c = 0; c < kMaxChains; ++c)
                if (c < C) d += sq(xv[c] - r[c * E + i]);
            vsum[(t - 1) * E + i] += d;
        }
#pragma unroll
        for (int c = 0; c < kMaxChains; ++c)
            if (c < C) ring[slot * CE + c * E + i] = xv[c];
    }
}

// split ESS of one component: var+ from the moments, rho_t = 1 - S_t / (M (n - t)) / (2 var+) read
// lag by lag until rho_{T+1} + rho_{T+2} < 0 (T odd, T + 2 <= Lp); truncated when no such T exists.  mcse = sqrt(var+ / ESS).
__device__ __forceinline__ void ess_component(const float* __restrict__ mean, const float* __restrict__ m2,
                                              const float* __restrict__ vsum, int64_t stride, int M, double n, int Lp,
                                              float& ess, float& mcse, bool& truncated) {
    double w, b;
    split_within_between(mean, m2, stride, M, n, w, b);
    const double varp = (n - 1.0) / n * w + b;
    const double mn = M * n;
    truncated = false;
    if (!(varp < (double)kDiagInf)) {  // non-finite moments (var+ >= 0 otherwise)
        ess = 0.0f;
        mcse = kDiagInf;
        return;
    }
    if (varp == 0.0) {  // constant everywhere
        ess = (float)mn;
        mcse = 0.0f;
        return;
    }
    const double scale = 1.0 / (2.0 * M * varp);
    auto rho = [&](int t) { return 1.0 - (double)vsum[(t - 1) * stride] * scale / (n - t); };
    double sum = rho(1);
    int T = 1;
    truncated = true;
    while (T + 2 <= Lp) {
        const double r1 = rho(T + 1), r2 = rho(T + 2);
        if (r1 + r2 < 0.0) {
            truncated = false;
            break;
        }
        sum += r1 + r2;
        T += 2;
    }
    const double tau = 1.0 + 2.0 * sum;
    if (!(fabs(tau) < (double)kDiagInf)) {  // non-finite lag sums
        ess = 0.0f;
        mcse = kDiagInf;
        return;
    }
    const double cap = mn * fmax(1.0, log10(mn));
    const double e = tau > mn / cap ? mn / tau : cap;
    ess = (float)e;
    mcse = (float)sqrt(varp / e);
}

__global__ __launch_bounds__(kBlock) void split_ess_kernel(const float* __restrict__ mean, const float* __restrict__ m2,
                                                           const float* __restrict__ vsum, int C, float n, int Lp,
                                                           const uint8_t* __restrict__ mask, float thr, float* __restrict__ ess,
                                                           float* __restrict__ mcse, double* __restrict__ partials, int64_t V) {
    __shared__ double smem[4 * (kBlock / kWave)];
    const int M = 2 * C;
    const int64_t seq = 3 * V;  // moments: sequence m at m * 3V; vsum: lag t at (t - 1) * 3V; component j at + j * V
    double acc[5] = {0.0, 0.0, 0.0, (double)kDiagInf, 0.0};  // voxels, ESS below thr, truncated, min ESS, sum of ESS
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        float e = kDiagInf, s = 0.0f;
        bool tr = false;
#pragma unroll 1
        for (int j = 0; j < 3; ++j) {
            float ej, sj;
            bool tj;
            ess_component(mean + j * V + v, m2 + j * V + v, vsum + j * V + v, seq, M, (double)n, Lp, ej, sj, tj);
            e = fminf(e, ej);
            s = fmaxf(s, sj);
            tr = tr || tj;
        }
        ess[v] = e;
        mcse[v] = s;
        if (!mask || mask[v]) {
            acc[0] += 1.0;
            acc[1] += e < thr ? 1.0 : 0.0;
            acc[2] += tr ? 1.0 : 0.0;
            acc[3] = fmin(acc[3], (double)e);
            acc[4] += (double)e;
        }
    }
    block_summary<true>(acc, smem);
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < 5; ++i) partials[(int64_t)blockIdx.x * 5 + i] = acc[i];
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
    hipLaunchKernelGGL(split_summary_reduce_kernel<false>, dim3(1), dim3(kBlock), 0, st, partials, blocks, summary);
}

void launch_chain_variogram(const float* x, float* ring, float* vsum, int C, int64_t E, int L, int k, hipStream_t st) {
    const bool vec = (E & 3) == 0 && (((uintptr_t)x | (uintptr_t)ring | (uintptr_t)vsum) & 15) == 0;
    const int64_t units = vec ? E / 4 : E;
    const dim3 grid((unsigned)std::min<int64_t>((units + kBlock - 1) / kBlock, kDiagMaxBlocks));
    const int lags = std::min(k - 1, L), slot = (k - 1) % L;
    if (vec) hipLaunchKernelGGL(chain_variogram_kernel<true>, grid, dim3(kBlock), 0, st, x, ring, vsum, C, E, L, lags, slot);
    else hipLaunchKernelGGL(chain_variogram_kernel<false>, grid, dim3(kBlock), 0, st, x, ring, vsum, C, E, L, lags, slot);
}

void launch_split_ess(const float* mean, const float* m2, const float* vsum, int C, int n, int L, const uint8_t* mask, float thr,
                      float* ess, float* mcse, double* summary, double* partials, int64_t V, hipStream_t st) {
    const int blocks = split_rhat_blocks(V);
    hipLaunchKernelGGL(split_ess_kernel, dim3(blocks), dim3(kBlock), 0, st, mean, m2, vsum, C, (float)n, std::min(L, n - 1),
                       mask, thr, ess, mcse, partials, V);
    hipLaunchKernelGGL(split_summary_reduce_kernel<true>, dim3(1), dim3(kBlock), 0, st, partials, blocks, summary);
}

}  // namespace irs
