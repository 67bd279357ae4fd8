// Landmark propagation (absent in the reference, which has no point-set operator): a sampled displacement evaluated at K
// arbitrary positions, the per-landmark posterior of the mapped points and their target registration error (DESIGN.md
// section 6, "Landmark propagation and TRE").
//
//  - transform_points: one thread per (chain, point), a grid-stride loop; the three channels are sampled by warp_sample
//    (warp_device.h) at the same position, so the three axis_taps are formed once and shared after inlining.  points / offset
//    stay AoS, 12-byte rows read once per chain.  The field is not restaged: at K << V the taps are scattered, an LDS tile buys nothing.
//  - update: one thread per landmark folds the C samples into its float64 state in chain order; each thread owns its
//    landmark: plain read-modify-writes, no atomics.
//  - finalize: one thread per landmark writes its row of the table (the eigen-solver is covariance_device.h's); the summary
//    stays in registers and is reduced by summary_device.h.
#include "covariance_device.h"
#include "kernels.h"
#include "summary_device.h"
#include "warp_device.h"

namespace irs {
namespace {

// integer sums {landmarks, landmarks with count == 0, landmarks with a finite pit}; doubles over the landmarks with count > 0
// {sum tre_of_mean, max tre_of_mean, sum tre_mean, max tre_max}.  The maxima never see a NaN.
struct LandmarkSummary {
    static constexpr int kInts = IRS_LANDMARK_SUMMARY_INTS, kFloats = IRS_LANDMARK_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 1 || j == 3 ? Col::Max : Col::Sum; }
};
using LandmarkAcc = SummaryAcc<LandmarkSummary>;

struct Scale3f {
    float s[3];
};

// points (K,3), field (C,3,V), offset (K,3) or nullptr; sampled / mapped (C,K,3), either may be nullptr
__global__ __launch_bounds__(kBlock) void transform_points_kernel(const float* __restrict__ points, const float* __restrict__ field,
                                                                  Scale3f sc, const float* __restrict__ offset,
                                                                  float* __restrict__ sampled, float* __restrict__ mapped, int K,
                                                                  int C, Vol vol) {
    const int64_t total = (int64_t)C * K;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int chain = (int)(t / K);
        const int64_t k3 = (t - (int64_t)chain * K) * 3;
        const float g[3] = {points[k3], points[k3 + 1], points[k3 + 2]};
        const float nan = __builtin_nanf("");
        float s[3] = {nan, nan, nan}, gm[3];
        if (isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2])) {  // a non-finite position reads no tap
            const float* src = field + (int64_t)chain * 3 * vol.V;
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] = warp_sample<false>(src + c * vol.V, g, vol, gm);
        }
        if (sampled) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sampled[t * 3 + c] = s[c];
        }
        if (mapped) {
#pragma unroll
            for (int c = 0; c < 3; ++c) mapped[t * 3 + c] = __fadd_rn(__fmul_rn(sc.s[c], s[c]), offset ? offset[k3 + c] : 0.0f);
        }
    }
}

// mapped (C,K,3), target (K,3) float32; the float64 state of one landmark per thread
__global__ __launch_bounds__(kBlock) void landmark_update_kernel(const float* __restrict__ mapped, const float* __restrict__ target,
                                                                 int C, int K, double* __restrict__ mean, double* __restrict__ comoment,
                                                                 double* __restrict__ tre_mean, double* __restrict__ tre_m2,
                                                                 double* __restrict__ tre_max, int32_t* __restrict__ count,
                                                                 int records_before) {
    for (int k = blockIdx.x * kBlock + threadIdx.x; k < K; k += gridDim.x * kBlock) {
        double mu[3] = {0.0, 0.0, 0.0}, M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, em = 0.0, e2 = 0.0, emax = 0.0;
        int n = 0;
        if (records_before > 0) {  // the first record of all overwrites: a fresh state is never read
#pragma unroll
            for (int a = 0; a < 3; ++a) mu[a] = mean[k * 3 + a];
#pragma unroll
            for (int a = 0; a < 6; ++a) M[a] = comoment[k * 6 + a];
            em = tre_mean[k], e2 = tre_m2[k], emax = tre_max[k], n = count[k];
        }
        const float tf[3] = {target[k * 3], target[k * 3 + 1], target[k * 3 + 2]};
        const bool target_ok = isfinite(tf[0]) && isfinite(tf[1]) && isfinite(tf[2]);
        for (int c = 0; c < C; ++c) {
            const float* xc = mapped + ((int64_t)c * K + k) * 3;
            const float xf[3] = {xc[0], xc[1], xc[2]};
            if (!(target_ok && isfinite(xf[0]) && isfinite(xf[1]) && isfinite(xf[2]))) continue;  // skipped, not counted
            const double x[3] = {(double)xf[0], (double)xf[1], (double)xf[2]};
            const double dn = (double)++n;
            const double d0 = x[0] - mu[0], d1 = x[1] - mu[1], d2 = x[2] - mu[2];
            mu[0] += d0 / dn;
            mu[1] += d1 / dn;
            mu[2] += d2 / dn;
            const double r0 = x[0] - mu[0], r1 = x[1] - mu[1], r2 = x[2] - mu[2];
            M[0] += d0 * r0;  // xx, xy, xz, yy, yz, zz
            M[1] += d0 * r1;
            M[2] += d0 * r2;
            M[3] += d1 * r1;
            M[4] += d1 * r2;
            M[5] += d2 * r2;
            const double t0 = x[0] - (double)tf[0], t1 = x[1] - (double)tf[1], t2 = x[2] - (double)tf[2];
            const double e = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
            const double de = e - em;
            em += de / dn;
            e2 += de * (e - em);
            emax = fmax(emax, e);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) mean[k * 3 + a] = mu[a];
#pragma unroll
        for (int a = 0; a < 6; ++a) comoment[k * 6 + a] = M[a];
        tre_mean[k] = em, tre_m2[k] = e2, tre_max[k] = emax, count[k] = n;
    }
}

// chi-square CDF with 3 degrees of freedom, closed form
__device__ __forceinline__ double chi2_cdf3(double x) {
    return erf(sqrt(0.5 * x)) - sqrt(2.0 * x / 3.14159265358979323846) * exp(-0.5 * x);
}

// the state -> out (K, IRS_LANDMARK_COLUMNS) and, per block, the summary columns
__global__ __launch_bounds__(kBlock) void landmark_finalize_kernel(const double* __restrict__ mean, const double* __restrict__ comoment,
                                                                   const double* __restrict__ tre_mean, const double* __restrict__ tre_m2,
                                                                   const double* __restrict__ tre_max, const int32_t* __restrict__ count,
                                                                   const float* __restrict__ target, int K, double* __restrict__ out,
                                                                   long long* __restrict__ ipart, double* __restrict__ fpart) {
    __shared__ LandmarkAcc smem[LandmarkAcc::kG];
    LandmarkAcc a = LandmarkAcc::identity();
    const double nan = __builtin_nan("");
    for (int k = blockIdx.x * kBlock + threadIdx.x; k < K; k += gridDim.x * kBlock) {
        const int n = count[k];
        double row[IRS_LANDMARK_COLUMNS];
#pragma unroll
        for (int j = 0; j < IRS_LANDMARK_COLUMNS; ++j) row[j] = nan;
        row[0] = (double)n;
        a.i[0] += 1;
        if (n > 0) {
            const double inv = 1.0 / (double)(n > 1 ? n - 1 : 1);
            const double* M = comoment + (int64_t)k * 6;
            const double r[3] = {mean[k * 3] - (double)target[k * 3], mean[k * 3 + 1] - (double)target[k * 3 + 1],
                                 mean[k * 3 + 2] - (double)target[k * 3 + 2]};
            double l0, l1, l2, e0[3], e1[3], e2[3];
            cov_eigen(M[0] * inv, M[3] * inv, M[5] * inv, M[1] * inv, M[2] * inv, M[4] * inv, l0, l1, l2, e0, e1, e2);
            row[1] = tre_mean[k];
            row[2] = sqrt(fmax(tre_m2[k], 0.0) * inv);
            row[3] = tre_max[k];
            row[4] = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            row[5] = sqrt(fmax(l0, 0.0));
            row[6] = sqrt(fmax(l1, 0.0));
            row[7] = sqrt(fmax(l2, 0.0));
            if (n >= 4 && l2 > 0.0) {  // in the eigenbasis: sum_i (r . e_i)^2 / l_i
                const double p0 = r[0] * e0[0] + r[1] * e0[1] + r[2] * e0[2];
                const double p1 = r[0] * e1[0] + r[1] * e1[1] + r[2] * e1[2];
                const double p2 = r[0] * e2[0] + r[1] * e2[1] + r[2] * e2[2];
                row[8] = p0 * p0 / l0 + p1 * p1 / l1 + p2 * p2 / l2;
                row[9] = chi2_cdf3(row[8]);
            }
            // a state somebody loaded may hold anything: the maxima must not see a NaN
            a.f[0] += row[4];
            if (isfinite(row[4])) a.f[1] = fmax(a.f[1], row[4]);
            a.f[2] += row[1];
            if (isfinite(row[3])) a.f[3] = fmax(a.f[3], row[3]);
            a.i[2] += isfinite(row[9]);
        } else {
            a.i[1] += 1;
        }
#pragma unroll
        for (int j = 0; j < IRS_LANDMARK_COLUMNS; ++j) out[(int64_t)k * IRS_LANDMARK_COLUMNS + j] = row[j];
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, blockIdx.x);
}

}  // namespace

void launch_transform_points(const float* points, int K, const float* displacement, const float* scale, const float* offset,
                             float* sampled, float* mapped, int C, Vol vol, hipStream_t st) {
    const int blocks = (int)std::min<int64_t>(((int64_t)C * K + kBlock - 1) / kBlock, 4096);
    const Scale3f sc = {{scale[0], scale[1], scale[2]}};
    hipLaunchKernelGGL(transform_points_kernel, dim3(blocks), dim3(kBlock), 0, st, points, displacement, sc, offset, sampled, mapped,
                       K, C, vol);
}

void launch_landmark_update(const float* mapped, const float* target, int C, int K, double* mean, double* comoment, double* tre_mean,
                            double* tre_m2, double* tre_max, int32_t* count, int records_before, hipStream_t st) {
    const int blocks = std::min((K + kBlock - 1) / kBlock, 4096);
    hipLaunchKernelGGL(landmark_update_kernel, dim3(blocks), dim3(kBlock), 0, st, mapped, target, C, K, mean, comoment, tre_mean,
                       tre_m2, tre_max, count, records_before);
}

void launch_landmark_finalize(const double* mean, const double* comoment, const double* tre_mean, const double* tre_m2,
                              const double* tre_max, const int32_t* count, const float* target, int K, double* out,
                              long long* isummary, double* fsummary, void* ws, hipStream_t st) {
    const SummaryPartials<LandmarkSummary> part(K, ws, IRS_LANDMARK_WS_BYTES);
    hipLaunchKernelGGL(landmark_finalize_kernel, dim3(part.blocks), dim3(kBlock), 0, st, mean, comoment, tre_mean, tre_m2, tre_max,
                       count, target, K, out, part.ipart, part.fpart);
    part.reduce(isummary, fsummary, st);
}

}  // namespace irs
