// Device arithmetic of the known-transformation validation (truth_kernels.hip): the per-voxel error of one sample against the
// truth, and the per-voxel calibration of a displacement covariance state against it.  Everything is in double with every
// operation rounded on its own (the __d*_rn intrinsics: nothing to contract), in the order include/irsgmcmc.h writes out, so
// that a float64 restatement on the host forms the same bits.  No transcendental: sqrt is the correctly rounded one.
#pragma once
#include "summary_device.h"

namespace irs {

// {voxels, voxels with a non-finite q}; {sum r, sum q, max r} over the finite ones
struct TruthUpdate {
    static constexpr int kInts = IRS_TRUTH_UPDATE_INTS, kFloats = IRS_TRUTH_UPDATE_FLOATS;
    static constexpr Col kind(int j) { return j == 2 ? Col::Max : Col::Sum; }
};
// {voxels, non-finite voxels, raised voxels}; {sum err, sum err2, max err, sum dist2, max dist2, sum v, sum z_x, z_y, z_z}
struct TruthSummary {
    static constexpr int kInts = IRS_TRUTH_SUMMARY_INTS, kFloats = IRS_TRUTH_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 2 || j == 4 ? Col::Max : Col::Sum; }
};
// one reliability bin: {voxels}; {sum v, sum err2}
struct TruthReliability {
    static constexpr int kInts = IRS_TRUTH_RELIABILITY_INTS, kFloats = IRS_TRUTH_RELIABILITY_FLOATS;
    static constexpr Col kind(int) { return Col::Sum; }
};

__device__ __forceinline__ bool truth_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN, +-inf
__device__ __forceinline__ bool truth_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// one masked voxel of one chain folded into its accumulator: e_c = s_c (u_c - t_c), q = (e_x^2 + e_y^2) + e_z^2, r = sqrt(q)
__device__ __forceinline__ void truth_error_fold(const float (&u)[3], const float (&t)[3], const double (&s)[3],
                                                 SummaryAcc<TruthUpdate>& a) {
    const double ex = __dmul_rn(s[0], __dsub_rn((double)u[0], (double)t[0]));
    const double ey = __dmul_rn(s[1], __dsub_rn((double)u[1], (double)t[1]));
    const double ez = __dmul_rn(s[2], __dsub_rn((double)u[2], (double)t[2]));
    const double q = __dadd_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)), __dmul_rn(ez, ez));
    a.i[0] += 1;
    if (truth_finite(q)) {
        const double r = __dsqrt_rn(q);
        a.f[0] += r;
        a.f[1] += q;
        a.f[2] = fmax(a.f[2], r);
    } else {
        a.i[1] += 1;
    }
}

struct TruthVoxel {
    bool finite, raised;
    double err2, dist2, v, z[3];
};

// a pivot below f^2 (or NaN) is raised to it
__device__ __forceinline__ double truth_pivot(double d, double f2, bool& raised) {
    if (!(d >= f2)) {
        raised = true;
        return f2;
    }
    return d;
}

// mean (3), comoment (6: xx, yy, zz, xy, xz, yz), truth (3) of one voxel -> its calibration terms (include/irsgmcmc.h:
// irs_truth_calibrate gives the operation order)
__device__ __forceinline__ TruthVoxel truth_calibrate_voxel(const float (&mu)[3], const float (&M)[6], const float (&t)[3],
                                                            const double (&s)[3], double nm1, double f2) {
    TruthVoxel o;
    o.finite = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) o.finite = o.finite && truth_finite(mu[c]) && truth_finite(t[c]);
#pragma unroll
    for (int c = 0; c < 6; ++c) o.finite = o.finite && truth_finite(M[c]);
    o.raised = false;
    double dl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dl[c] = __dmul_rn(s[c], __dsub_rn((double)mu[c], (double)t[c]));
    auto entry = [&](int a, int b, int k) { return __ddiv_rn(__dmul_rn(__dmul_rn(s[a], s[b]), (double)M[k]), nm1); };
    const double axx = __dadd_rn(entry(0, 0, 0), f2), ayy = __dadd_rn(entry(1, 1, 1), f2), azz = __dadd_rn(entry(2, 2, 2), f2);
    const double axy = entry(0, 1, 3), axz = entry(0, 2, 4), ayz = entry(1, 2, 5);
    const double d0 = truth_pivot(axx, f2, o.raised);
    const double l10 = __ddiv_rn(axy, d0), l20 = __ddiv_rn(axz, d0);
    const double d1 = truth_pivot(__dsub_rn(ayy, __dmul_rn(l10, axy)), f2, o.raised);
    const double w = __dsub_rn(ayz, __dmul_rn(l20, axy));
    const double l21 = __ddiv_rn(w, d1);
    const double d2 = truth_pivot(__dsub_rn(__dsub_rn(azz, __dmul_rn(l20, axz)), __dmul_rn(l21, w)), f2, o.raised);
    const double y0 = dl[0];
    const double y1 = __dsub_rn(dl[1], __dmul_rn(l10, y0));
    const double y2 = __dsub_rn(__dsub_rn(dl[2], __dmul_rn(l20, y0)), __dmul_rn(l21, y1));
    o.dist2 = __dadd_rn(__dadd_rn(__ddiv_rn(__dmul_rn(y0, y0), d0), __ddiv_rn(__dmul_rn(y1, y1), d1)), __ddiv_rn(__dmul_rn(y2, y2), d2));
    const double ex2 = __dmul_rn(dl[0], dl[0]), ey2 = __dmul_rn(dl[1], dl[1]), ez2 = __dmul_rn(dl[2], dl[2]);
    o.err2 = __dadd_rn(__dadd_rn(ex2, ey2), ez2);
    o.v = __dadd_rn(__dadd_rn(axx, ayy), azz);
    o.z[0] = __ddiv_rn(ex2, axx >= f2 ? axx : f2);
    o.z[1] = __ddiv_rn(ey2, ayy >= f2 ? ayy : f2);
    o.z[2] = __ddiv_rn(ez2, azz >= f2 ? azz : f2);
    o.finite = o.finite && truth_finite(o.dist2);
    return o;
}

// the number of the n edges that are <= x (edges increasing): the bin of x among n + 1 bins
__device__ __forceinline__ int truth_bin(const double* edges, int n, double x) {
    int b = 0;
    for (int e = 0; e < n; ++e) b += edges[e] <= x ? 1 : 0;
    return b;
}

}  // namespace irs
