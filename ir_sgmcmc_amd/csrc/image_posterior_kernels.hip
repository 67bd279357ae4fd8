// Image posterior (absent in the reference): per voxel, how the intensity of a volume on the moving image's grid varies when it
// is carried through every recorded transformation -- Welford mean / M2, minimum and maximum.
//
//  - update: one launch per recorded step for all C chains and all S volumes, one voxel per thread on the 64 x 4 voxel grid of
//    the pointwise kernels.  Per chain the thread reads its three transformation components and forms the three axis taps, the
//    eight corner offsets and the eight weights ONCE; every volume reuses them, so only the eight gathers and the fold differ
//    per volume and no warped intermediate exists.  The sampled value is warp_transformation_kernel's, expression for
//    expression (field_kernels.hip): bit-identical to irs_warp_transformation.  The state of a thread's volumes stays in
//    registers over the chain loop: loaded once, stored once, plain read-modify-writes (each thread owns its voxel).  Registers
//    need a compile-time volume count: blockIdx.z carries (volume group, plane), a group is kImagePosteriorGroup = 2 volumes and
//    the last one the TAIL = S - 2 (groups - 1) volumes the kernel is templated on.
//    Why two volumes per thread and not four: every volume of a thread is four state planes read and four written, so a wavefront
//    of four volumes keeps 32 separate streams going beside its 32 gathers per chain.  Measured on one MI355X, medians of
//    per-call device events, alternating builds twice (C = 2): 256^3, S = 8: 2.31 ms with four volumes per thread, 2.02 ms with
//    one (the taps and the 12 C bytes of transformation per voxel once per volume), 1.87 ms with two; S = 4: 1.21 / 1.08 /
//    1.00 ms; 128^3, S = 8: 0.287 / 0.236 / 0.227 ms.  Two keeps most of the reuse at half the streams.
//  - finalize (per volume): a grid-stride stream over voxels writes the std, range and z maps; the summary over the mask stays
//    in registers and is reduced by summary_device.h.
#include "kernels.h"
#include "summary_device.h"

namespace irs {
namespace {

constexpr int kGroup = kImagePosteriorGroup;  // volumes per thread: 8 state registers + 8 offsets + 8 weights, 16 gathers in flight

// the summary columns: integer sums {voxels, non-finite voxels, |z| > 2, |z| > 3}; then doubles {sum mean, sum std, max std,
// max range, sum z^2, max |z|}
struct ImagePosteriorSummary {
    static constexpr int kInts = IRS_IMAGE_POSTERIOR_SUMMARY_INTS, kFloats = IRS_IMAGE_POSTERIOR_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return (j == 2 || j == 3 || j == 5) ? Col::Max : Col::Sum; }
};
using ImAcc = SummaryAcc<ImagePosteriorSummary>;

// NV volumes at `vols` (stride V) through the C transformations at `t`, folded into the NV state planes at mean / m2 / low /
// high (stride V) of voxel p
template <int NV>
__device__ __forceinline__ void fold_volumes(const float* __restrict__ vols, const float* __restrict__ t, int C,
                                             float* __restrict__ mean, float* __restrict__ m2, float* __restrict__ low,
                                             float* __restrict__ high, int records_before, int64_t p, const Vol vol) {
    float mu[NV], s[NV], lo[NV], hi[NV];
    if (records_before > 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int64_t q = (int64_t)v * vol.V + p;
            mu[v] = mean[q];
            s[v] = m2[q];
            lo[v] = low[q];
            hi[v] = high[q];
        }
    }
    for (int c = 0; c < C; ++c) {
        const float* tc = t + (int64_t)c * 3 * vol.V;
        const AxisTap tx = axis_tap(tc[p], vol.W), ty = axis_tap(tc[vol.V + p], vol.H), tz = axis_tap(tc[2 * vol.V + p], vol.D);
        // 32-bit element offsets inside one volume (V < 2^30: dims_ok), corners in z, y, x order
        unsigned off[8];
        float w[8];
#pragma unroll
        for (int cz = 0; cz < 2; ++cz)
#pragma unroll
            for (int cy = 0; cy < 2; ++cy) {
                const unsigned rowoff = ((unsigned)(cz ? tz.i1 : tz.i0) * (unsigned)vol.H + (unsigned)(cy ? ty.i1 : ty.i0)) * (unsigned)vol.W;
#pragma unroll
                for (int cx = 0; cx < 2; ++cx) {
                    off[cz * 4 + cy * 2 + cx] = rowoff + (unsigned)(cx ? tx.i1 : tx.i0);
                    w[cz * 4 + cy * 2 + cx] = __fmul_rn(__fmul_rn(cx ? tx.w1 : tx.w0, cy ? ty.w1 : ty.w0), cz ? tz.w1 : tz.w0);
                }
            }
        const int k = records_before + c + 1;
        const float kf = (float)k;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const float* src = vols + (int64_t)v * vol.V;
            float x = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) x = __fadd_rn(x, __fmul_rn(src[off[j]], w[j]));
            if (k == 1) {  // the first record of all overwrites whatever the state held
                mu[v] = lo[v] = hi[v] = x;
                s[v] = 0.0f;
            } else {
                const float d = x - mu[v];
                mu[v] += d / kf;
                s[v] += d * (x - mu[v]);
                lo[v] = fminf(lo[v], x);
                hi[v] = fmaxf(hi[v], x);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int64_t q = (int64_t)v * vol.V + p;
        mean[q] = mu[v];
        m2[q] = s[v];
        low[q] = lo[v];
        high[q] = hi[v];
    }
}

// volumes (S,V), t (C,3,V), mean / m2 / low / high (S,V) float32; grid z = groups * D, TAIL = volumes of the last group
template <int TAIL>
__global__ __launch_bounds__(kBlock) void image_posterior_update_kernel(const float* __restrict__ volumes, int groups,
                                                                        const float* __restrict__ t, int C, float* __restrict__ mean,
                                                                        float* __restrict__ m2, float* __restrict__ low,
                                                                        float* __restrict__ high, int records_before, Vol vol) {
    IRS_VOXEL(vol, group, x, y, z, p);
    (void)x; (void)y; (void)z;
    const int64_t base = (int64_t)group * kGroup * vol.V;  // across volumes: 64-bit
    if (group < groups - 1)  // block-uniform
        fold_volumes<kGroup>(volumes + base, t, C, mean + base, m2 + base, low + base, high + base, records_before, p, vol);
    else
        fold_volumes<TAIL>(volumes + base, t, C, mean + base, m2 + base, low + base, high + base, records_before, p, vol);
}

// mean / m2 / low / high (V) float32 of one volume after n records, reference (V) or nullptr -> std, range, z (V) float32 and,
// per block, the summary columns over the mask: one row of partials
__global__ __launch_bounds__(kBlock) void image_posterior_finalize_kernel(const float* __restrict__ mean, const float* __restrict__ m2,
                                                                          const float* __restrict__ low, const float* __restrict__ high,
                                                                          int64_t V, int n, const float* __restrict__ reference,
                                                                          float std_floor, const uint8_t* __restrict__ mask,
                                                                          float* __restrict__ std_out, float* __restrict__ range_out,
                                                                          float* __restrict__ z_out, long long* __restrict__ ipart,
                                                                          double* __restrict__ fpart) {
    __shared__ ImAcc smem[ImAcc::kG];
    ImAcc a = ImAcc::identity();
    const float denom = (float)(n > 1 ? n - 1 : 1), floor2 = std_floor * std_floor;
    const float nan = __builtin_nanf("");
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        const float mu = mean[v];
        const bool finite = isfinite(mu);
        const float sd = finite ? sqrtf(m2[v] / denom) : nan;
        const float rg = finite ? high[v] - low[v] : nan;
        float z = nan;
        if (reference && finite) z = (reference[v] - mu) / sqrtf(sd * sd + floor2);
        std_out[v] = sd;
        range_out[v] = rg;
        if (reference) z_out[v] = z;
        if (!mask || mask[v]) {
            a.i[0] += 1;
            a.i[1] += !finite;
            if (finite) {
                a.f[0] += (double)mu;
                a.f[1] += (double)sd;
                a.f[2] = fmax(a.f[2], (double)sd);
                a.f[3] = fmax(a.f[3], (double)rg);
                if (z == z) {  // 0 / 0 (reference == mean, no spread and no floor) enters no z column
                    const double az = fabs((double)z);
                    a.i[2] += az > 2.0;
                    a.i[3] += az > 3.0;
                    a.f[4] += az * az;
                    a.f[5] = fmax(a.f[5], az);
                }
            }
        }
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, blockIdx.x);
}

// without a reference the two z columns are NaN (the counts are 0 already)
__global__ void image_posterior_no_reference_kernel(double* __restrict__ fsummary) {
    fsummary[4] = fsummary[5] = __builtin_nan("");
}

}  // namespace

void launch_image_posterior_update(const float* volumes, int S, const float* t, int C, float* mean, float* m2, float* low,
                                   float* high, int records_before, Vol vol, hipStream_t st) {
    const int groups = (S + kGroup - 1) / kGroup, tail = S - kGroup * (groups - 1);
    const dim3 grid = vox_grid(vol, groups);
#define IRS_IMAGE_UPDATE(TAIL)                                                                                                   \
    hipLaunchKernelGGL(image_posterior_update_kernel<TAIL>, grid, dim3(kBlock), 0, st, volumes, groups, t, C, mean, m2, low, high, \
                       records_before, vol)
    static_assert(kGroup == 2, "one case per tail below");
    if (tail == 1)
        IRS_IMAGE_UPDATE(1);
    else
        IRS_IMAGE_UPDATE(2);
#undef IRS_IMAGE_UPDATE
}

void launch_image_posterior_finalize(const float* mean, const float* m2, const float* low, const float* high, int64_t V, int n,
                                     const float* reference, float std_floor, const uint8_t* mask, float* std_out, float* range_out,
                                     float* z_out, long long* isummary, double* fsummary, void* ws, hipStream_t st) {
    const SummaryPartials<ImagePosteriorSummary> part(V, ws, IRS_IMAGE_POSTERIOR_WS_BYTES);
    hipLaunchKernelGGL(image_posterior_finalize_kernel, dim3(part.blocks), dim3(kBlock), 0, st, mean, m2, low, high, V, n, reference,
                       std_floor, mask, std_out, range_out, z_out, part.ipart, part.fpart);
    part.reduce(isummary, fsummary, st);
    if (!reference) hipLaunchKernelGGL(image_posterior_no_reference_kernel, dim3(1), dim3(1), 0, st, fsummary);
}

}  // namespace irs
