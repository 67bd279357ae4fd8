// Displacement covariance posterior (absent in the reference): per voxel, the Welford mean and the six co-moments of the
// displacement over the recorded samples, and at the end the principal spreads, the major direction and the fractional
// anisotropy of the 3 x 3 sample covariance.
//
//  - update: one launch per recorded step for all C chains, one voxel per thread on the 64 x 4 voxel grid of the pointwise
//    kernels.  The thread loads the nine state values once, folds the chains into them in order (covariance_device.h) and
//    stores once; each thread owns its voxel: plain read-modify-writes, no atomics.  (Four consecutive voxels per thread with
//    16-byte accesses measured no faster: DESIGN.md section 6.)
//  - finalize: a grid-stride stream over voxels diagonalises the covariance in double (a fixed number of cyclic Jacobi
//    sweeps, no data-dependent trip count) and writes the seven planes; the summary over the mask stays in registers and is
//    reduced by summary_device.h.
#include "covariance_device.h"
#include "kernels.h"
#include "summary_device.h"

namespace irs {
namespace {

// the summary columns: integer sums {voxels, voxels with a non-finite state}; then doubles over the stored float32 maps of
// the finite voxels {sum std[0], max std[0], sum sqrt(std0^2 + std1^2 + std2^2), sum anisotropy, max anisotropy,
// sum |direction_x|, |direction_y|, |direction_z|}.  The maxima never see a NaN.
struct CovarianceSummary {
    static constexpr int kInts = IRS_COVARIANCE_SUMMARY_INTS, kFloats = IRS_COVARIANCE_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 1 || j == 4 ? Col::Max : Col::Sum; }
};
using CovAcc = SummaryAcc<CovarianceSummary>;

// x (C,3,V) float32; mean (3,V), comoment (6,V) float32.  One voxel per thread.
__global__ __launch_bounds__(kBlock) void covariance_update_kernel(const float* __restrict__ x, int C, float* __restrict__ mean,
                                                                   float* __restrict__ comoment, int records_before, Vol vol) {
    IRS_VOXEL(vol, plane_, xx_, yy_, zz_, p);
    (void)plane_;
    float mu[3] = {0.0f, 0.0f, 0.0f}, M[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (records_before > 0) {  // the first record of all overwrites: a fresh state is never read
#pragma unroll
        for (int a = 0; a < 3; ++a) mu[a] = mean[a * vol.V + p];
#pragma unroll
        for (int a = 0; a < 6; ++a) M[a] = comoment[a * vol.V + p];
    }
    for (int c = 0; c < C; ++c) {
        const float* xc = x + (int64_t)c * 3 * vol.V + p;
        cov_fold(xc[0], xc[vol.V], xc[2 * vol.V], records_before + c + 1, mu, M);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) mean[a * vol.V + p] = mu[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) comoment[a * vol.V + p] = M[a];
}

struct CovScale {
    double s[3];
};

// mean (3,V), comoment (6,V) after n records -> std (3,V), direction (3,V), anisotropy (V) float32 and, per block, the summary
// columns over the mask
__global__ __launch_bounds__(kBlock) void covariance_finalize_kernel(const float* __restrict__ mean, const float* __restrict__ comoment,
                                                                     int64_t V, int n, CovScale scale, const uint8_t* __restrict__ mask,
                                                                     float* __restrict__ stdev, float* __restrict__ direction,
                                                                     float* __restrict__ anisotropy, long long* __restrict__ ipart,
                                                                     double* __restrict__ fpart) {
    __shared__ CovAcc smem[CovAcc::kG];
    CovAcc a = CovAcc::identity();
    const double inv = 1.0 / (double)(n > 1 ? n - 1 : 1);
    const double sc[3] = {scale.s[0], scale.s[1], scale.s[2]};
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        float mu[3], M[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[c] = mean[c * V + v];
#pragma unroll
        for (int c = 0; c < 6; ++c) M[c] = comoment[c * V + v];
        const CovMaps o = cov_maps(mu, M, inv, sc);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            stdev[c * V + v] = o.std[c];
            direction[c * V + v] = o.dir[c];
        }
        anisotropy[v] = o.fa;
        if (!mask || mask[v]) {
            a.i[0] += 1;
            if (o.finite) {
                const double s0 = o.std[0], s1 = o.std[1], s2 = o.std[2];
                a.f[0] += s0;
                a.f[1] = fmax(a.f[1], s0);
                a.f[2] += sqrt(s0 * s0 + s1 * s1 + s2 * s2);
                a.f[3] += (double)o.fa;
                a.f[4] = fmax(a.f[4], (double)o.fa);
                a.f[5] += fabs((double)o.dir[0]);
                a.f[6] += fabs((double)o.dir[1]);
                a.f[7] += fabs((double)o.dir[2]);
            } else {
                a.i[1] += 1;
            }
        }
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, blockIdx.x);
}

}  // namespace

void launch_covariance_update(const float* x, int C, float* mean, float* comoment, int records_before, Vol vol, hipStream_t st) {
    hipLaunchKernelGGL(covariance_update_kernel, vox_grid(vol, 1), dim3(kBlock), 0, st, x, C, mean, comoment, records_before, vol);
}

void launch_covariance_finalize(const float* mean, const float* comoment, int64_t V, int n, const float* scale, const uint8_t* mask,
                                float* stdev, float* direction, float* anisotropy, long long* isummary, double* fsummary, void* ws,
                                hipStream_t st) {
    const SummaryPartials<CovarianceSummary> part(V, ws, IRS_COVARIANCE_WS_BYTES);
    const CovScale sc{{(double)scale[0], (double)scale[1], (double)scale[2]}};
    hipLaunchKernelGGL(covariance_finalize_kernel, dim3(part.blocks), dim3(kBlock), 0, st, mean, comoment, V, n, sc, mask, stdev,
                       direction, anisotropy, part.ipart, part.fpart);
    part.reduce(isummary, fsummary, st);
}

}  // namespace irs
