// Posterior maps on the image's own voxel grid (absent in the reference): per native voxel the counts of every structure over
// the recorded nearest-neighbour warps of the moving segmentation, and the Welford mean / M2, minimum and maximum of the trilinear
// sample of the moving image.  The samples are irs_native_warp's: the steps of native_device.h, call for
// call as native_warp_kernel makes them, so the label is the value it writes to seg_out and the intensity the bits it writes to
// im_out.  Neither warped volume exists.
//
//  - update: one launch per recorded step for all C chains.  A wavefront walks rows (y, z) of the native volume and its lanes
//    stride along x, so a thread owns its voxels and every access to the state is coalesced; the grid depends on the native
//    extents only.  Per chain, in order c = 0 .. C - 1, the thread forms the displacement and the source position ONCE; the
//    label part rounds it (half to even), reads the segmentation (0 outside the native box) and adds 1 to the count plane of its
//    structure -- a plain read-modify-write --, the image part gathers the eight taps and folds the sample into the four state
//    values, which stay in registers over the chain loop: read once, written once.  The fold is irs_image_posterior_update's
//    recurrence with every operation an explicit round-to-nearest intrinsic (nothing is contracted into an FMA).
//    The per-record volumes are counted per block in LDS with wave_count, which every lane of a wavefront has to reach: the
//    lanes beyond the end of a row pass j = -1.  The block partials (C x K int32) go to the workspace; label_kernels.hip's fold
//    adds them in block order and folds the Welford update in chain order.
//  - templated on {labels, image}: a caller that wants one part pays nothing for the other.
#include <algorithm>

#include "label_device.h"
#include "native_device.h"

namespace irs {
namespace {

// 16 wavefronts per block and at most one block per CU: the chip holds as many wavefronts as with 1024 blocks of four, and the
// one-block fold behind the launch adds a quarter of the rows of partials (measured at 182 x 218 x 182, C = 2, K = 15: the fold
// took 62 us of a 0.395 ms step with 1024 rows; the step is 0.344 ms with 256)
constexpr int kNativeBlock = 1024;
constexpr int kNativePosteriorMaxBlocks = 256;
constexpr int kRowsPerBlock = kNativeBlock / kWave;

template <bool LAB, bool IMG>
__global__ __launch_bounds__(kNativeBlock) void native_posterior_kernel(const float* __restrict__ u, const float* __restrict__ im,
                                                                  const int16_t* __restrict__ seg, int64_t moving_stride, int C,
                                                                  SurfLabels lab, int K, int32_t* __restrict__ counts,
                                                                  int32_t* __restrict__ partials, float* __restrict__ mean,
                                                                  float* __restrict__ m2, float* __restrict__ low,
                                                                  float* __restrict__ high, int records_before, NativeGeom gm,
                                                                  Vol vol) {
    __shared__ int volume[LAB ? IRS_MAX_CHAINS * IRS_MAX_LABELS : 1];
    const int CK = C * K;
    if (LAB) {
        for (int i = threadIdx.x; i < CK; i += kNativeBlock) volume[i] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned nhw = (unsigned)(vol.H * vol.W), nw = (unsigned)vol.W;
    const int rows = vol.H * vol.D;
    // the row and the x base are the same for the 64 lanes of a wavefront: they run the loops together
    for (int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6); row < rows; row += gridDim.x * kRowsPerBlock) {
        const int z = row / vol.H, y = row - z * vol.H;
        for (int x0 = 0; x0 < vol.W; x0 += kWave) {
            const int x = x0 + lane;
            const bool owns = x < vol.W;  // false beyond the end of the row: nothing read or written, j = -1 below
            const int64_t vox = (int64_t)row * vol.W + x;
            const int idx[3] = {z, y, x};  // axis order (D, H, W)
            float mu = 0.0f, s = 0.0f, lo = 0.0f, hi = 0.0f;
            if (IMG && owns && records_before > 0) {
                mu = mean[vox];
                s = m2[vox];
                lo = low[vox];
                hi = high[vox];
            }
            for (int c = 0; c < C; ++c) {
                int j = -1;
                if (owns) {
                    float uc[3], r[3];
                    native_displacement(u, c, idx, gm, uc);
                    native_source(uc, idx, gm, r);
                    const int64_t mov = (int64_t)c * moving_stride;
                    if (LAB) {
                        unsigned off = 0;
                        bool in = true;
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            const BoxIndex b = box_index((int)nearbyintf(r[a]), gm.p[a], gm.n[a]);
                            off += (unsigned)b.i * (a == 0 ? nhw : (a == 1 ? nw : 1u));
                            in = in && b.in;
                        }
                        j = structure_of(in ? seg[mov + off] : (int16_t)0, lab, K);
                        if (j >= 0) counts[(int64_t)j * vol.V + vox] += 1;
                    }
                    if (IMG) {
                        const float v = native_trilinear(im + mov, native_taps(r, gm), gm.fill);
                        const int k = records_before + c + 1;
                        if (k == 1) {  // the first record of all overwrites whatever the state held
                            mu = lo = hi = v;
                            s = 0.0f;
                        } else {
                            const float d = __fsub_rn(v, mu);
                            mu = __fadd_rn(mu, __fdiv_rn(d, (float)k));
                            s = __fadd_rn(s, __fmul_rn(d, __fsub_rn(v, mu)));
                            lo = fminf(lo, v);
                            hi = fmaxf(hi, v);
                        }
                    }
                }
                if (LAB) wave_count(j, volume + c * K);
            }
            if (IMG && owns) {
                mean[vox] = mu;
                m2[vox] = s;
                low[vox] = lo;
                high[vox] = hi;
            }
        }
    }
    if (LAB) {
        __syncthreads();
        for (int i = threadIdx.x; i < CK; i += kNativeBlock) partials[(int64_t)blockIdx.x * CK + i] = volume[i];
    }
}

}  // namespace

int native_posterior_blocks(const NativeGeom& gm) {
    const int64_t rows = (int64_t)gm.n[0] * gm.n[1];
    return (int)std::min<int64_t>((rows + kRowsPerBlock - 1) / kRowsPerBlock, kNativePosteriorMaxBlocks);
}

void launch_native_posterior_update(const float* u, const float* im, const int16_t* seg, int64_t moving_stride, const SurfLabels& lab,
                                    int K, int32_t* counts, double* volume, int32_t* partials, float* mean, float* m2, float* low,
                                    float* high, int records_before, const NativeGeom& gm, int C, hipStream_t st) {
    const Vol vol = make_vol(gm.n[0], gm.n[1], gm.n[2]);
    const int blocks = native_posterior_blocks(gm);
#define IRS_NATIVE_POSTERIOR(LAB, IMG)                                                                                            \
    hipLaunchKernelGGL((native_posterior_kernel<LAB, IMG>), dim3(blocks), dim3(kNativeBlock), 0, st, u, im, seg, moving_stride, C, lab, \
                       K, counts, partials, mean, m2, low, high, records_before, gm, vol)
    if (seg && im)
        IRS_NATIVE_POSTERIOR(true, true);
    else if (seg)
        IRS_NATIVE_POSTERIOR(true, false);
    else
        IRS_NATIVE_POSTERIOR(false, true);
#undef IRS_NATIVE_POSTERIOR
    if (seg) launch_label_volume_fold(partials, blocks, C, K, volume, records_before, st);
}

}  // namespace irs
