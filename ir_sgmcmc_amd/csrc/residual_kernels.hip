// Residual model check (the numbers behind the reference's log_hist_res figure, logger/visualization.py:64-86; DESIGN.md
// section 6): is the likelihood -- a zero-mean Gaussian mixture over the residual z -- a fair description of the residuals
// it is applied to, and where in the volume is it not.
//
//  - histogram: one launch for all chains, blockIdx.y the chain.  A grid-stride stream over the chain's voxels; each thread
//    reads z and the mask once (5 bytes per voxel and chain), four voxels per 16-byte load when V % 4 == 0 and the bases are
//    aligned (the base of chain c is c V floats), one otherwise.  A voxel takes part when the mask is set (or absent) and z is
//    finite.  Binning in fp32: t = (z + h) * inv_w -- a sum, then a product: nothing to contract -- b = min(B - 1, max(0,
//    floor(t))); |z| > h counts as clipped.  The bin goes to a uint32 histogram in LDS, one copy per wavefront (B <= 512:
//    8 KB for the four), so that the wavefronts of a block never meet on an address.  Inside a wavefront they do: LCC
//    residuals of flat background are exactly 0, whole wavefronts land in one bin and 64 adds to one LDS address serialise --
//    hist_add (histogram_device.h) then adds their number with one lane (the switch similarity_aggregate; 0: plain atomics
//    always).  The three integer counts and the four doubles {sum z, sum z^2, sum z^4, max |z|} stay in registers
//    (SummaryAcc, summary_device.h).  At the end the non-zero bins go to the int64 histogram of the caller with integer
//    atomics -- exact, so their order does not matter -- and one row of partials per block to the workspace.
//  - finish: one block per chain folds the chain's partial rows (thread i rows i, i + 256, ... in order, then the block
//    reduction: lanes by the shuffle butterfly, the wavefronts in order) and overwrites or merges the caller's counts and sums:
//    integer adds, ONE double add per sum, fmax for the maximum.
//  - nll update / finalize: the per-voxel posterior mean of -log p(z) under a mixture passed by value; each thread owns its
//    voxels, no atomics; the masked summary through summary_device.h.
// Two identical call sequences are bit-identical: integer histogram, fixed-order double sums, a grid per chain that depends on V
// only -- so chain c of a C-chain call is the single-chain call on that chain, bit for bit.
#include <algorithm>

#include "histogram_device.h"
#include "kernels.h"
#include "summary_device.h"

namespace irs {
namespace {

// integer sums {voxels taking part, masked voxels with a non-finite z, voxels with |z| > half_range}; doubles {sum z, sum z^2,
// sum z^4, max |z|} over the voxels taking part
struct ResSummary {
    static constexpr int kInts = 3, kFloats = 4;
    static constexpr Col kind(int j) { return j == 3 ? Col::Max : Col::Sum; }
};
using ResAcc = SummaryAcc<ResSummary>;

// over the mask: integer sums {voxels, voxels with count == 0}; doubles over the others {sum of mean, max of mean}
struct ResMapSummary {
    static constexpr int kInts = IRS_RESIDUAL_MAP_SUMMARY_INTS, kFloats = IRS_RESIDUAL_MAP_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 0 ? Col::Sum : Col::Max; }
};
using ResMapAcc = SummaryAcc<ResMapSummary>;

constexpr int kResWaves = kBlock / kWave;

struct ResVoxel {
    bool take;
    int bin;
};

// one voxel into the register sums; -> whether it takes part and its bin
__device__ __forceinline__ ResVoxel res_voxel(float z, bool masked, const ResBins& bn, ResAcc& a) {
    const bool finite = isfinite(z);
    const bool take = masked && finite;
    a.i[1] += masked && !finite;
    // clamped as floats: floor(t) of a finite residual far outside the range need not fit an int
    const int b = (int)fminf(fmaxf(floorf(__fmul_rn(__fadd_rn(z, bn.half_range), bn.inv_w)), 0.0f), (float)(bn.bins - 1));
    if (take) {
        const double dz = (double)z, z2 = dz * dz;  // exact: 24-bit significands
        a.i[0] += 1;
        a.i[2] += fabsf(z) > bn.half_range;
        a.f[0] += dz;
        a.f[1] += z2;
        a.f[2] += z2 * z2;
        a.f[3] = fmax(a.f[3], fabs(dz));
    }
    return {take, take ? b : 0};
}

// z (C,V); mask (V) or nullptr; hist (C,B) int64, ready to be added to; row chain * gridDim.x + blockIdx.x of the partials.
// VEC: V % 4 == 0, z 16-byte and mask 4-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void residual_histogram_kernel(const float* __restrict__ residuals,
                                                                    const uint8_t* __restrict__ mask, int64_t V, ResBins bn,
                                                                    bool aggregate, long long* __restrict__ hist,
                                                                    long long* __restrict__ ipart, double* __restrict__ fpart) {
    __shared__ uint32_t h[kResWaves][IRS_RESIDUAL_MAX_BINS];  // one copy per wavefront
    __shared__ ResAcc smem[ResAcc::kG];
    for (int i = threadIdx.x; i < kResWaves * IRS_RESIDUAL_MAX_BINS; i += kBlock) (&h[0][0])[i] = 0;
    __syncthreads();

    const int chain = blockIdx.y;
    const float* z = residuals + (int64_t)chain * V;
    uint32_t* hw = h[threadIdx.x / kWave];
    ResAcc a = ResAcc::identity();
    const int64_t units = VEC ? V >> 2 : V;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // the trip count is the wavefront's: the ballots of hist_add see every lane
    for (int64_t u0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1)); u0 < units; u0 += stride) {
        const int64_t u = u0 + (threadIdx.x & (kWave - 1));
        const bool in = u < units;
        if (VEC) {
            float4 zv = {0.0f, 0.0f, 0.0f, 0.0f};
            uint32_t k = 0;
            if (in) {
                zv = reinterpret_cast<const float4*>(z)[u];
                k = mask ? reinterpret_cast<const uint32_t*>(mask)[u] : 0x01010101u;
            }
            const float za[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const ResVoxel vx = res_voxel(za[s], ((k >> (8 * s)) & 0xFFu) != 0, bn, a);
                hist_add(hw, vx.take, vx.bin, aggregate);
            }
        } else {
            float zs = 0.0f;
            bool k = false;
            if (in) {
                zs = z[u];
                k = mask ? mask[u] != 0 : true;
            }
            const ResVoxel vx = res_voxel(zs, k, bn, a);
            hist_add(hw, vx.take, vx.bin, aggregate);
        }
    }
    __syncthreads();
    unsigned long long* hc = reinterpret_cast<unsigned long long*>(hist) + (int64_t)chain * bn.bins;
    for (int i = threadIdx.x; i < bn.bins; i += kBlock) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < kResWaves; ++w) c += h[w][i];
        if (c) atomicAdd(&hc[i], (unsigned long long)c);
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, (int64_t)chain * gridDim.x + blockIdx.x);
}

// one block per chain: the chain's `nblocks` rows of partials -> counts (C,3) int64, sums (C,4) double, overwritten
// (records_before == 0) or merged
__global__ __launch_bounds__(kBlock) void residual_histogram_finish_kernel(const long long* __restrict__ ipart,
                                                                           const double* __restrict__ fpart, int nblocks,
                                                                           long long* __restrict__ counts,
                                                                           double* __restrict__ sums, int records_before) {
    __shared__ ResAcc smem[ResAcc::kG];
    const int chain = blockIdx.x;
    ResAcc a = ResAcc::identity();
    for (int b = threadIdx.x; b < nblocks; b += kBlock) a.merge(ResAcc::load(ipart, fpart, (int64_t)chain * nblocks + b));
    a.block_reduce(smem);
    if (threadIdx.x == 0) {
        if (records_before > 0) a.merge(ResAcc::load(counts, sums, chain));  // one add per column, fmax for the maximum
        a.store(counts, sums, chain);
    }
}

// z (C,V) -> mean (V) float32, count (V) int32: each thread owns its voxels, the chains folded in order, a non-finite z skipped
__global__ __launch_bounds__(kBlock) void residual_nll_update_kernel(const float* __restrict__ residuals, int C, int64_t V,
                                                                     ResMixture mix, float* __restrict__ mean,
                                                                     int32_t* __restrict__ count, int records_before) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        float mu = 0.0f;
        int n = 0;
        if (records_before > 0) {
            mu = mean[v];
            n = count[v];
        }
        for (int c = 0; c < C; ++c) {
            const float zf = residuals[(int64_t)c * V + v];
            if (!isfinite(zf)) continue;
            const double z = (double)zf;
            double a[IRS_MAX_COMPONENTS];
            double m = -INFINITY;
#pragma unroll
            for (int k = 0; k < IRS_MAX_COMPONENTS; ++k) {
                if (k < mix.K) {
                    const double t = z * mix.inv_std[k];
                    a[k] = mix.log_weight[k] - 0.5 * (t * t);
                    m = fmax(m, a[k]);
                }
            }
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < IRS_MAX_COMPONENTS; ++k)
                if (k < mix.K) s += exp(a[k] - m);
            const float nll = (float)(-(m + log(s)));
            ++n;
            mu = __fadd_rn(mu, __fsub_rn(nll, mu) / (float)n);
        }
        mean[v] = mu;
        count[v] = n;
    }
}

__global__ __launch_bounds__(kBlock) void residual_nll_finalize_kernel(const float* __restrict__ mean,
                                                                       const int32_t* __restrict__ count, int64_t V,
                                                                       const uint8_t* __restrict__ mask,
                                                                       long long* __restrict__ ipart, double* __restrict__ fpart) {
    __shared__ ResMapAcc smem[ResMapAcc::kG];
    ResMapAcc a = ResMapAcc::identity();
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[v]) continue;
        a.i[0] += 1;
        if (count[v] > 0) {  // every sample folded in was finite: so is the mean
            const double mu = (double)mean[v];
            a.f[0] += mu;
            a.f[1] = fmax(a.f[1], mu);
        } else {
            a.i[1] += 1;
        }
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, blockIdx.x);
}

}  // namespace

void launch_residual_histogram(const float* residuals, const uint8_t* mask, int64_t V, int C, const ResBins& bn, long long* hist,
                               long long* counts, double* sums, int records_before, void* ws, hipStream_t st) {
    const bool vec = (V & 3) == 0 && ((uintptr_t)residuals & 15) == 0 && ((uintptr_t)mask & 3) == 0;
    const int64_t units = vec ? V >> 2 : V;
    // blocks per chain: by V (and the alignment) only, whatever C
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((units + kBlock - 1) / kBlock, IRS_RESIDUAL_MAX_BLOCKS));
    long long* ipart = (long long*)ws;
    double* fpart = (double*)(ipart + (size_t)ResSummary::kInts * blocks * C);
    const bool aggregate = global_knobs().similarity_aggregate != 0;
    if (records_before == 0) (void)hipMemsetAsync(hist, 0, (size_t)C * bn.bins * sizeof(long long), st);
    if (vec)
        hipLaunchKernelGGL(residual_histogram_kernel<true>, dim3(blocks, C), dim3(kBlock), 0, st, residuals, mask, V, bn, aggregate,
                           hist, ipart, fpart);
    else
        hipLaunchKernelGGL(residual_histogram_kernel<false>, dim3(blocks, C), dim3(kBlock), 0, st, residuals, mask, V, bn, aggregate,
                           hist, ipart, fpart);
    hipLaunchKernelGGL(residual_histogram_finish_kernel, dim3(C), dim3(kBlock), 0, st, ipart, fpart, blocks, counts, sums,
                       records_before);
}

static int residual_stream_blocks(int64_t n) { return (int)std::min<int64_t>((n + kBlock - 1) / kBlock, 4096); }

void launch_residual_nll_update(const float* residuals, int C, int64_t V, const ResMixture& mix, float* mean, int32_t* count,
                                int records_before, hipStream_t st) {
    hipLaunchKernelGGL(residual_nll_update_kernel, dim3(residual_stream_blocks(V)), dim3(kBlock), 0, st, residuals, C, V, mix, mean,
                       count, records_before);
}

void launch_residual_nll_finalize(const float* mean, const int32_t* count, int64_t V, const uint8_t* mask, long long* isummary,
                                  double* fsummary, void* ws, hipStream_t st) {
    const SummaryPartials<ResMapSummary> part(V, ws, IRS_RESIDUAL_MAP_WS_BYTES);
    hipLaunchKernelGGL(residual_nll_finalize_kernel, dim3(part.blocks), dim3(kBlock), 0, st, mean, count, V, mask, part.ipart,
                       part.fpart);
    part.reduce(isummary, fsummary, st);
}

}  // namespace irs
