// The arithmetic the kernels of the mutual-information data term share (mi_kernels.hip; include/irsgmcmc.h: irs_mi_fwd): the bin
// of the fixed intensity, the cubic B-spline coordinate of the moving intensity, the four Parzen weights, their derivatives and
// their Q30 fixed-point form.  Everything about the moving intensity is double with every operation rounded ONCE -- the file is
// built with -ffp-contract=on, so products and sums go through __dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn as hist_bin's do in
// float -- which lets a numpy float64 restatement reproduce the integers of the histogram bit for bit.
#pragma once
#include "histogram_device.h"

namespace irs {

constexpr int kMiQ = 30;  // fixed-point bits of a Parzen weight: every voxel adds exactly 2^30 to its histogram

// k0: the taps are the moving bins k0 - 1 .. k0 + 2, always inside [0, bins - 1]; u in [0, 1]: the position between taps k0 and
// k0 + 1; inside: the unclamped coordinate lies in [1, bins - 2] (outside the gradient is 0 and the voxel counts as clipped)
struct MiCoord {
    int k0;
    double u;
    bool inside;
};

// t_raw = (m - m_lo) * m_scale + 1 with m_scale = (bins - 3) / (m_hi - m_lo) formed on the host in double; t = clamp(t_raw, 1,
// bins - 2); k0 = min(floor(t), bins - 3); u = t - k0.  A NaN gives k0 = 1, u = 0, inside = false (fmax / fmin drop it).
__device__ __forceinline__ MiCoord mi_coord(float m, const MiBins& bn) {
    const double top = (double)(bn.bins - 2);
    const double t_raw = __dadd_rn(__dmul_rn(__dsub_rn((double)m, bn.m_lo), bn.m_scale), 1.0);
    const double t = fmin(fmax(t_raw, 1.0), top);
    const int k0 = min((int)floor(t), bn.bins - 3);
    return {k0, __dsub_rn(t, (double)k0), t_raw >= 1.0 && t_raw <= top};
}

// w = ((1-u)^3, 3u^3 - 6u^2 + 4, -3u^3 + 3u^2 + 3u + 1, u^3) / 6, in this order of operations
__device__ __forceinline__ void mi_weights(double u, double (&w)[4]) {
    const double om = __dsub_rn(1.0, u), u2 = __dmul_rn(u, u), u3 = __dmul_rn(u2, u);
    const double a3 = __dmul_rn(3.0, u3), b3 = __dmul_rn(3.0, u2);
    w[0] = __ddiv_rn(__dmul_rn(__dmul_rn(om, om), om), 6.0);
    w[1] = __ddiv_rn(__dadd_rn(__dsub_rn(a3, __dmul_rn(6.0, u2)), 4.0), 6.0);
    w[2] = __ddiv_rn(__dadd_rn(__dadd_rn(__dsub_rn(b3, a3), __dmul_rn(3.0, u)), 1.0), 6.0);
    w[3] = __ddiv_rn(u3, 6.0);
}

// w' = (-(1-u)^2 / 2, 1.5u^2 - 2u, -1.5u^2 + u + 0.5, u^2 / 2): they sum to 0
__device__ __forceinline__ void mi_weight_derivatives(double u, double (&d)[4]) {
    const double om = __dsub_rn(1.0, u), u2 = __dmul_rn(u, u), c = __dmul_rn(1.5, u2);
    d[0] = -__dmul_rn(__dmul_rn(om, om), 0.5);
    d[1] = __dsub_rn(c, __dmul_rn(2.0, u));
    d[2] = __dadd_rn(__dsub_rn(u, c), 0.5);
    d[3] = __dmul_rn(u2, 0.5);
}

// q_j = round(w_j 2^30) (to nearest, ties to even) for j = 0, 2, 3; q_1 takes the rest of 2^30
__device__ __forceinline__ void mi_fixed_point(const double (&w)[4], unsigned long long (&q)[4]) {
    const double one = (double)(1ull << kMiQ);
    q[0] = (unsigned long long)rint(__dmul_rn(w[0], one));
    q[2] = (unsigned long long)rint(__dmul_rn(w[2], one));
    q[3] = (unsigned long long)rint(__dmul_rn(w[3], one));
    q[1] = (1ull << kMiQ) - q[0] - q[2] - q[3];
}

// one voxel: whether it takes part (mask set, both intensities finite), its fixed bin a and its moving coordinate
struct MiVoxel {
    bool take;
    int a;
    MiCoord m;
};
__device__ __forceinline__ MiVoxel mi_voxel(float f, float m, bool masked, const MiBins& bn) {
    MiVoxel v;
    v.take = masked && isfinite(f) && isfinite(m);
    v.a = hist_bin(f, bn.f_lo, bn.f_inv, (float)(bn.bins - 1));
    v.m = mi_coord(m, bn);
    return v;
}

}  // namespace irs
