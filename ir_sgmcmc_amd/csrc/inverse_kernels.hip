// Inverse transformation and inverse-consistency error (absent in the reference, which only ever evaluates the forward map;
// DESIGN.md section 6).
//
//  - negate: -v into the scratch of irs_svf_exp_inverse; the squaring steps of exp(-v) are the launches of the forward
//    exponential (exp_kernels.hip), unchanged.
//  - composition: per chain and voxel r = d_a(x) + trilinear(d_b)(t_a(x)), the three channels of d_b sampled by warp_sample
//    (warp_device.h) at the same position, so the three axis_taps are formed once and shared after inlining.  The kernel is
//    gather-bound (3 channels x 8 taps per voxel): a grid-stride stream over the voxels of one chain per block row, planar
//    layout, every stream read and write coalesced along x, no LDS, no atomics.  The per-chain summary over the mask stays in
//    registers and is reduced by summary_device.h: one row of partials per block, one reduce per chain.
//  - update / finalize: Welford mean and running maximum of the norm maps, and their masked summary.
#include "kernels.h"
#include "summary_device.h"
#include "warp_device.h"

namespace irs {
namespace {

// per chain over the mask: integer sums {voxels, voxels with a non-finite norm}; doubles {sum norm, sum norm^2, max norm} over
// the finite ones (fmax never sees a NaN)
struct IceSummary {
    static constexpr int kInts = IRS_ICE_SUMMARY_INTS, kFloats = IRS_ICE_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 2 ? Col::Max : Col::Sum; }
};
using IceAcc = SummaryAcc<IceSummary>;

// of the two maps over the mask: integer sums {voxels, voxels with a non-finite mean, voxels with peak > threshold}; doubles
// {sum mean, max mean} over the voxels with a finite mean and {max peak} over those with a finite peak
struct IceMapSummary {
    static constexpr int kInts = IRS_ICE_MAP_SUMMARY_INTS, kFloats = IRS_ICE_MAP_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 0 ? Col::Sum : Col::Max; }
};
using IceMapAcc = SummaryAcc<IceMapSummary>;

struct Scale3f {
    float s[3];
};

__global__ __launch_bounds__(kBlock) void negate_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) out[i] = -in[i];
}

// t_a, d_a, d_b (C,3,V); mask (mask_chains,V) or nullptr; residual (C,3,V) or nullptr; norm (C,V) or nullptr.  blockIdx.y is
// the chain; row blockIdx.x of the chain's partials (part_stride 8-byte words apart from the next chain's)
__global__ __launch_bounds__(kBlock) void inverse_consistency_kernel(const float* __restrict__ t_a, const float* __restrict__ d_a,
                                                                     const float* __restrict__ d_b, Scale3f sc,
                                                                     const uint8_t* __restrict__ mask, int64_t mask_stride,
                                                                     float* __restrict__ residual, float* __restrict__ norm,
                                                                     long long* __restrict__ ipart, double* __restrict__ fpart,
                                                                     int64_t part_stride, Vol vol) {
    __shared__ IceAcc smem[IceAcc::kG];
    IceAcc a = IceAcc::identity();
    const int chain = blockIdx.y;
    const int64_t cb3 = (int64_t)chain * 3 * vol.V;
    const float* src = d_b + cb3;
    const uint8_t* m = mask ? mask + (int64_t)chain * mask_stride : nullptr;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < vol.V; v += (int64_t)gridDim.x * kBlock) {
        const float g[3] = {t_a[cb3 + v], t_a[cb3 + vol.V + v], t_a[cb3 + 2 * vol.V + v]};
        float gm[3], r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = __fadd_rn(d_a[cb3 + c * vol.V + v], warp_sample<false>(src + c * vol.V, g, vol, gm));
        if (residual) {
#pragma unroll
            for (int c = 0; c < 3; ++c) residual[cb3 + c * vol.V + v] = r[c];
        }
        const float sx = __fmul_rn(sc.s[0], r[0]), sy = __fmul_rn(sc.s[1], r[1]), sz = __fmul_rn(sc.s[2], r[2]);
        const float nv = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(sx, sx), __fmul_rn(sy, sy)), __fmul_rn(sz, sz)));
        if (norm) norm[(int64_t)chain * vol.V + v] = nv;
        if (!m || m[v]) {
            a.i[0] += 1;
            if (isfinite(nv)) {
                a.f[0] += (double)nv;
                a.f[1] += (double)nv * (double)nv;
                a.f[2] = fmax(a.f[2], (double)nv);
            } else {
                a.i[1] += 1;
            }
        }
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart + chain * part_stride, fpart + chain * part_stride, blockIdx.x);
}

// norm (C,V) -> mean, peak (V): each thread owns its voxels, the chains folded in order
__global__ __launch_bounds__(kBlock) void inverse_consistency_update_kernel(const float* __restrict__ norm, int C, int64_t V,
                                                                            float* __restrict__ mean, float* __restrict__ peak,
                                                                            int records_before) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        float mu = 0.0f, pk = __builtin_nanf("");
        if (records_before > 0) {
            mu = mean[v];
            pk = peak[v];
        }
        for (int c = 0; c < C; ++c) {
            const float x = norm[(int64_t)c * V + v];
            const int k = records_before + c + 1;
            mu = k == 1 ? x : __fadd_rn(mu, __fsub_rn(x, mu) / (float)k);
            if (isfinite(x)) pk = isnan(pk) ? x : fmaxf(pk, x);
        }
        mean[v] = mu;
        peak[v] = pk;
    }
}

__global__ __launch_bounds__(kBlock) void inverse_consistency_finalize_kernel(const float* __restrict__ mean,
                                                                              const float* __restrict__ peak, int64_t V,
                                                                              const uint8_t* __restrict__ mask, float threshold,
                                                                              long long* __restrict__ ipart,
                                                                              double* __restrict__ fpart) {
    __shared__ IceMapAcc smem[IceMapAcc::kG];
    IceMapAcc a = IceMapAcc::identity();
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[v]) continue;
        const float mu = mean[v], pk = peak[v];
        a.i[0] += 1;
        if (isfinite(mu)) {
            a.f[0] += (double)mu;
            a.f[1] = fmax(a.f[1], (double)mu);
        } else {
            a.i[1] += 1;
        }
        if (isfinite(pk)) {
            a.i[2] += pk > threshold;
            a.f[2] = fmax(a.f[2], (double)pk);
        }
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, blockIdx.x);
}

int stream_blocks(int64_t n) { return (int)std::min<int64_t>((n + kBlock - 1) / kBlock, 4096); }

}  // namespace

void launch_negate(const float* in, float* out, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(negate_kernel, dim3(stream_blocks(n)), dim3(kBlock), 0, st, in, out, n);
}

void launch_inverse_consistency(const float* t_a, const float* d_a, const float* d_b, const float* scale, const uint8_t* mask,
                                int mask_chains, float* residual, float* norm, long long* isummary, double* fsummary, void* ws,
                                int C, Vol vol, hipStream_t st) {
    // every chain has the same share of the workspace whatever C is: the grid depends on the volume only
    constexpr int chunk = IRS_ICE_WS_BYTES / IRS_MAX_CHAINS;
    const SummaryPartials<IceSummary> part(vol.V, ws, chunk);
    const Scale3f sc = {{scale[0], scale[1], scale[2]}};
    hipLaunchKernelGGL(inverse_consistency_kernel, dim3(part.blocks, C), dim3(kBlock), 0, st, t_a, d_a, d_b, sc, mask,
                       mask_chains == C && C > 1 ? vol.V : (int64_t)0, residual, norm, part.ipart, part.fpart,
                       (int64_t)(chunk / 8), vol);
    for (int c = 0; c < C; ++c) {
        const SummaryPartials<IceSummary> pc(vol.V, (char*)ws + (size_t)c * chunk, chunk);
        pc.reduce(isummary + (size_t)c * IceSummary::kInts, fsummary + (size_t)c * IceSummary::kFloats, st);
    }
}

void launch_inverse_consistency_update(const float* norm, int C, int64_t V, float* mean, float* peak, int records_before,
                                       hipStream_t st) {
    hipLaunchKernelGGL(inverse_consistency_update_kernel, dim3(stream_blocks(V)), dim3(kBlock), 0, st, norm, C, V, mean, peak,
                       records_before);
}

void launch_inverse_consistency_finalize(const float* mean, const float* peak, int64_t V, const uint8_t* mask, float threshold,
                                         long long* isummary, double* fsummary, void* ws, hipStream_t st) {
    const SummaryPartials<IceMapSummary> part(V, ws, IRS_ICE_MAP_WS_BYTES);
    hipLaunchKernelGGL(inverse_consistency_finalize_kernel, dim3(part.blocks), dim3(kBlock), 0, st, mean, peak, V, mask, threshold,
                       part.ipart, part.fpart);
    part.reduce(isummary, fsummary, st);
}

}  // namespace irs
