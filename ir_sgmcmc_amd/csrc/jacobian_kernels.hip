// Jacobian posterior maps (absent in the reference): per voxel, how often the sampled transformation folds and the mean and
// spread of log det J over the records that do not.
//
//  - update: one launch per recorded step for all C chains, one voxel per thread on the 64 x 4 voxel grid of the pointwise
//    kernels.  The thread loads its folds / mean / m2 once, folds every chain's det (jacobian_device.h: the arithmetic of the
//    per-sample fold count) into them in chain order, and stores once.  Each thread owns its voxel: plain read-modify-writes.
//  - finalize: a grid-stride stream over voxels writes the three maps; the summary over the mask stays in registers (exact
//    integer counts, double sums of the stored float32 values, min / max) and is reduced by summary_device.h.
#include "jacobian_device.h"
#include "kernels.h"
#include "summary_device.h"

namespace irs {
namespace {

// the summary columns: integer sums {voxels, folded voxels, always folded, fold records}; then doubles {max fold_prob,
// min logJ_mean, max logJ_mean, sum logJ_std, max logJ_std}.  fmin / fmax never see a NaN here: voxels without a valid
// record are left out of float columns 1 .. 4.
struct JacobianSummary {
    static constexpr int kInts = IRS_JACOBIAN_SUMMARY_INTS, kFloats = IRS_JACOBIAN_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 1 ? Col::Min : j == 3 ? Col::Sum : Col::Max; }
};
using JacAcc = SummaryAcc<JacobianSummary>;

// t (C,3,V) float32; folds (V) int32, mean / m2 (V) float32.  A record is folded when !(det > 0): det <= 0 or NaN.
__global__ __launch_bounds__(kBlock) void jacobian_update_kernel(const float* __restrict__ t, int C, int32_t* __restrict__ folds,
                                                                 float* __restrict__ mean, float* __restrict__ m2,
                                                                 int records_before, Vol vol) {
    IRS_VOXEL(vol, plane_, x, y, z, p);
    (void)plane_;
    // the first record of all overwrites the fold count, a voxel's first valid record its moments
    int f = records_before > 0 ? folds[p] : 0;
    int k = max(records_before - f, 0);  // valid records so far
    float mu = mean[p], s = m2[p];
    for (int c = 0; c < C; ++c) {
        const float det = det_jacobian(t + (int64_t)c * 3 * vol.V, p, x, y, z, vol);
        if (!(det > 0.0f)) {
            ++f;
            continue;
        }
        const float v = logf(det);
        ++k;
        if (k == 1) {
            mu = v;
            s = 0.0f;
        } else {
            const float d = v - mu;
            mu += d / (float)k;
            s += d * (v - mu);
        }
    }
    folds[p] = f;
    mean[p] = mu;
    m2[p] = s;
}

// folds (V) int32, mean / m2 (V) float32 after n records -> fold_prob, logJ_mean, logJ_std (V) float32 and, per block, the
// summary columns over the mask: one row of partials
__global__ __launch_bounds__(kBlock) void jacobian_finalize_kernel(const int32_t* __restrict__ folds, const float* __restrict__ mean,
                                                                   const float* __restrict__ m2, int64_t V, int n,
                                                                   const uint8_t* __restrict__ mask, float* __restrict__ fold_prob,
                                                                   float* __restrict__ logj_mean, float* __restrict__ logj_std,
                                                                   long long* __restrict__ ipart, double* __restrict__ fpart) {
    __shared__ JacAcc smem[JacAcc::kG];
    JacAcc a = JacAcc::identity();
    const double inv_n = 1.0 / (double)n;
    const float nan = __builtin_nanf("");
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        const int f = folds[v];
        const int64_t k = (int64_t)n - f;  // valid records
        const float fp = (float)((double)f * inv_n);
        const float lm = k >= 1 ? mean[v] : nan;
        const float ls = k >= 1 ? sqrtf(m2[v] / (float)(k > 1 ? k - 1 : 1)) : nan;
        fold_prob[v] = fp;
        logj_mean[v] = lm;
        logj_std[v] = ls;
        if (!mask || mask[v]) {
            a.i[0] += 1;
            a.i[1] += f > 0;
            a.i[2] += k < 1;
            a.i[3] += f;
            a.f[0] = fmax(a.f[0], (double)fp);
            if (k >= 1) {
                a.f[1] = fmin(a.f[1], (double)lm);
                a.f[2] = fmax(a.f[2], (double)lm);
                a.f[3] += (double)ls;
                a.f[4] = fmax(a.f[4], (double)ls);
            }
        }
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, blockIdx.x);
}

}  // namespace

void launch_jacobian_update(const float* t, int C, int32_t* folds, float* mean, float* m2, int records_before, Vol vol,
                            hipStream_t st) {
    hipLaunchKernelGGL(jacobian_update_kernel, vox_grid(vol, 1), dim3(kBlock), 0, st, t, C, folds, mean, m2, records_before, vol);
}

void launch_jacobian_finalize(const int32_t* folds, const float* mean, const float* m2, int64_t V, int n, const uint8_t* mask,
                              float* fold_prob, float* logj_mean, float* logj_std, long long* isummary, double* fsummary,
                              void* ws, hipStream_t st) {
    const SummaryPartials<JacobianSummary> part(V, ws, IRS_JACOBIAN_WS_BYTES);
    hipLaunchKernelGGL(jacobian_finalize_kernel, dim3(part.blocks), dim3(kBlock), 0, st, folds, mean, m2, V, n, mask, fold_prob,
                       logj_mean, logj_std, part.ipart, part.fpart);
    part.reduce(isummary, fsummary, st);
}

}  // namespace irs
