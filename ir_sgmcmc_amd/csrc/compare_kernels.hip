// Posterior comparison (absent in the reference, which writes the VI and the MCMC displacement std side by side and leaves the
// comparison to the reader): per voxel, the distances between the 3-D Gaussians fitted to two Welford states of the
// displacement -- the mean shift, the log ratio of the total spreads, the Bures distance of the covariances and the Jeffreys
// divergence ("Posterior comparison"; the arithmetic is compare_device.h).
//
// One grid-stride stream over voxels, one voxel per thread and iteration: 18 loads, three 3 x 3 eigen-solves in double of a
// fixed number of cyclic Jacobi sweeps (no data-dependent trip count), 4 stores; the summary over the mask stays in registers
// and is reduced by summary_device.h.
#include "compare_device.h"
#include "kernels.h"
#include "summary_device.h"

namespace irs {
namespace {

// the summary columns: integer sums {voxels, voxels with a non-finite state, voxels with a floored eigenvalue, voxels with
// log_std_ratio < 0}; then doubles over the stored float32 maps of the finite voxels {sum, max shift; sum, min, max
// log_std_ratio; sum, max bures; sum, max w2 = sqrt(shift^2 + bures^2); sum, max jeffreys; sum tr S_A; sum tr S_B}.  The
// extrema never see a NaN.
struct CompareSummary {
    static constexpr int kInts = IRS_COMPARE_SUMMARY_INTS, kFloats = IRS_COMPARE_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 1 || j == 4 || j == 6 || j == 8 || j == 10 ? Col::Max : j == 3 ? Col::Min : Col::Sum; }
};
using CompareAcc = SummaryAcc<CompareSummary>;

struct CompareScale {
    double s[3];
};

// mean_x (3,V), comoment_x (6,V) after n_x records -> shift, log_std_ratio, bures, jeffreys (V) float32 and, per block, the
// summary columns over the mask
__global__ __launch_bounds__(kBlock) void posterior_compare_kernel(const float* __restrict__ mean_a, const float* __restrict__ comoment_a,
                                                                   int n_a, const float* __restrict__ mean_b,
                                                                   const float* __restrict__ comoment_b, int n_b, int64_t V,
                                                                   CompareScale scale, double floor2, const uint8_t* __restrict__ mask,
                                                                   float* __restrict__ shift, float* __restrict__ log_std_ratio,
                                                                   float* __restrict__ bures, float* __restrict__ jeffreys,
                                                                   long long* __restrict__ ipart, double* __restrict__ fpart) {
    __shared__ CompareAcc smem[CompareAcc::kG];
    CompareAcc a = CompareAcc::identity();
    const double inv_a = 1.0 / (double)(n_a - 1), inv_b = 1.0 / (double)(n_b - 1);
    const double sc[3] = {scale.s[0], scale.s[1], scale.s[2]};
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        float mu_a[3], M_a[6], mu_b[3], M_b[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) mu_a[c] = mean_a[c * V + v], mu_b[c] = mean_b[c * V + v];
#pragma unroll
        for (int c = 0; c < 6; ++c) M_a[c] = comoment_a[c * V + v], M_b[c] = comoment_b[c * V + v];
        const CompareMaps o = compare_maps(mu_a, M_a, inv_a, mu_b, M_b, inv_b, sc, floor2);
        shift[v] = o.shift;
        log_std_ratio[v] = o.log_std_ratio;
        bures[v] = o.bures;
        jeffreys[v] = o.jeffreys;
        if (!mask || mask[v]) {
            a.i[0] += 1;
            if (o.finite) {
                const double sh = o.shift, lr = o.log_std_ratio, bu = o.bures, je = o.jeffreys;
                const double w2 = sqrt(sh * sh + bu * bu);
                a.i[2] += o.floored ? 1 : 0;
                a.i[3] += o.log_std_ratio < 0.0f ? 1 : 0;
                a.f[0] += sh;
                a.f[1] = fmax(a.f[1], sh);
                a.f[2] += lr;
                a.f[3] = fmin(a.f[3], lr);
                a.f[4] = fmax(a.f[4], lr);
                a.f[5] += bu;
                a.f[6] = fmax(a.f[6], bu);
                a.f[7] += w2;
                a.f[8] = fmax(a.f[8], w2);
                a.f[9] += je;
                a.f[10] = fmax(a.f[10], je);
                a.f[11] += o.tr_a;
                a.f[12] += o.tr_b;
            } else {
                a.i[1] += 1;
            }
        }
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, blockIdx.x);
}

}  // namespace

void launch_posterior_compare(const float* mean_a, const float* comoment_a, int n_a, const float* mean_b, const float* comoment_b,
                              int n_b, int64_t V, const float* scale, double std_floor, const uint8_t* mask, float* shift,
                              float* log_std_ratio, float* bures, float* jeffreys, long long* isummary, double* fsummary, void* ws,
                              hipStream_t st) {
    const SummaryPartials<CompareSummary> part(V, ws, IRS_COMPARE_WS_BYTES);
    const CompareScale sc{{(double)scale[0], (double)scale[1], (double)scale[2]}};
    const double floor2 = (double)std_floor * (double)std_floor;
    hipLaunchKernelGGL(posterior_compare_kernel, dim3(part.blocks), dim3(kBlock), 0, st, mean_a, comoment_a, n_a, mean_b, comoment_b,
                       n_b, V, sc, floor2, mask, shift, log_std_ratio, bures, jeffreys, part.ipart, part.fpart);
    part.reduce(isummary, fsummary, st);
}

}  // namespace irs
