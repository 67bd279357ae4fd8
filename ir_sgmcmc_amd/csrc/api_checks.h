// Argument checks shared by the entry points of include/irsgmcmc.h (api_ops.hip, api_ctx.hip, slab.hip).  Every `*_ok` returns
// true when the argument is fine; the ones that take `who` -- the entry point's name -- leave the refusal in irs_last_error().
#pragma once
#include <math.h>
#include <string.h>

#include "ctx.h"

namespace irs {

inline bool dims_ok(int C, int D, int H, int W) {
    // < 2^30 voxels per volume: kernels address within a volume with 32-bit byte offsets (a 1024^3 transition would need
    // 240 GB of workspace anyway)
    return C >= 1 && D >= 2 && H >= 2 && W >= 2 && (int64_t)D * H * W < ((int64_t)1 << 30);
}

inline bool lcc_ok(int s, int D, int H, int W) { return (s == 1 || s == 2) && D > 2 * s && H > 2 * s && W > 2 * s; }

inline bool chain_count_ok(int C) { return C >= 1 && C <= IRS_MAX_CHAINS; }
inline bool broadcast_ok(int Cf, int C) { return Cf == 1 || Cf == C; }  // an array of one chain serves all, or there is one per chain
inline bool positive_finite(float v) { return v > 0.0f && isfinite(v); }

// the two numbers of the SGHMC sampler (sghmc_device.h): friction in (0, 1], temperature >= 0 and finite
inline bool sghmc_numbers_ok(const char* who, float friction, float temperature) {
    if (!(friction > 0.0f && friction <= 1.0f)) return !fail("%s: friction = %g, a value in (0, 1] needed", who, (double)friction);
    return (temperature >= 0.0f && isfinite(temperature)) || !fail("%s: temperature = %g, a finite value >= 0 needed", who, (double)temperature);
}

// (fail() returns 1: `!fail(...)` is "refused")
inline bool chains_ok(const char* who, int C) { return chain_count_ok(C) || !fail("%s: C = %d chains, 1..%d", who, C, IRS_MAX_CHAINS); }

// a recorder takes C records on top of `records_before`; `overflow` words what happens beyond `ceiling`
inline bool records_ok(const char* who, int records_before, int C, int64_t ceiling, const char* overflow) {
    if (records_before < 0) return !fail("%s: records_before = %d < 0", who, records_before);
    return (int64_t)records_before + C <= ceiling || !fail("%s: %d records + %d chains %s", who, records_before, C, overflow);
}

// three per-axis factors (`name`: scale, width ...), each finite and > 0
inline bool positive3(const char* who, const char* name, const float* values) {
    for (int a = 0; a < 3; ++a)
        if (!positive_finite(values[a])) return !fail("%s: %s[%d] = %g, a finite value > 0 needed", who, name, a, (double)values[a]);
    return true;
}

// `hint`: the function or constant that tells the size
inline bool workspace_ok(const char* who, size_t have, size_t need, const char* hint) {
    return have >= need || !fail("%s: workspace of %zu bytes, %zu needed (%s)", who, have, need, hint);
}

// the geometry of a native-resolution warp (irs_native_warp, irs_native_warp_cubic) -> gm (out_scale 0, fill unset) and the
// voxels of the native volume; `min_native`: the smallest native extent the caller takes
inline bool native_geometry_ok(const char* who, int C, const int32_t* dims, const int32_t* native, const int32_t* padding,
                               int min_native, NativeGeom& gm, int64_t& voxels) {
    voxels = 1;
    for (int a = 0; a < 3; ++a) {
        const int64_t P = (int64_t)native[a] + 2 * (int64_t)padding[a];
        if (native[a] < min_native) return !fail("%s: native[%d] = %d < %d", who, a, native[a], min_native);
        if (padding[a] < 0) return !fail("%s: padding[%d] = %d < 0", who, a, padding[a]);
        if (P < 2) return !fail("%s: padded extent %lld of axis %d, >= 2 needed", who, (long long)P, a);
        if (dims[a] < 2) return !fail("%s: dims[%d] = %d < 2", who, a, dims[a]);
        if (P >= ((int64_t)1 << 24)) return !fail("%s: padded extent %lld of axis %d is not exact in float32", who, (long long)P, a);
        voxels *= native[a];
        gm.n[a] = native[a];
        gm.p[a] = padding[a];
        gm.P[a] = (int)P;
        gm.m[a] = dims[a];
        gm.grid_step[a] = (float)((double)(dims[a] - 1) / (double)(P - 1));
        gm.half_extent[a] = 0.5f * (float)(P - 1);
        gm.out_scale[a] = 0.0f;
        if (voxels >= ((int64_t)1 << 30)) return !fail("%s: the native volume must have fewer than 2^30 voxels", who);
    }
    if (!dims_ok(C, dims[0], dims[1], dims[2])) return !fail("%s: bad dims", who);
    // the launch is one block row per (chain, plane) and per four rows of a plane
    return ((int64_t)native[0] * C <= 65535 && (native[1] + 3) / 4 <= 65535) ||
           !fail("%s: native shape (%d, %d, %d) x %d chains exceeds the launch grid", who, native[0], native[1], native[2], C);
}

// the volume of a cubic B-spline call: every extent >= 2 (the mirror needs two samples), fewer than 2^30 voxels, and `volumes`
// volumes of it within the launch grid (one block row per volume and plane, and per four rows of a plane)
inline bool bspline_volume_ok(const char* who, int volumes, int D, int H, int W) {
    if (D < 2 || H < 2 || W < 2) return !fail("%s: dims (%d, %d, %d), every one >= 2 needed", who, D, H, W);
    if ((int64_t)D * H * W >= ((int64_t)1 << 30)) return !fail("%s: the volume must have fewer than 2^30 voxels", who);
    return ((int64_t)D * volumes <= 65535 && (H + 3) / 4 <= 65535) ||
           !fail("%s: dims (%d, %d, %d) x %d volumes exceed the launch grid", who, D, H, W, volumes);
}

// the volumes of a mask call (mask_kernels.hip): C >= 1 of them, every extent >= 1, fewer than 2^30 voxels each (labels and union-
// find parents are int32 voxel indices) and one launch row per volume and plane
inline bool mask_volumes_ok(const char* who, int C, int D, int H, int W) {
    if (C < 1) return !fail("%s: C = %d volumes, at least 1 needed", who, C);
    if (D < 1 || H < 1 || W < 1) return !fail("%s: dims (%d, %d, %d), every one >= 1 needed", who, D, H, W);
    if ((int64_t)D * H * W >= ((int64_t)1 << 30)) return !fail("%s: the volume must have fewer than 2^30 voxels", who);
    return (int64_t)C * D <= 65535 || !fail("%s: %d volumes of %d planes are more than the 65535 rows of one launch", who, C, D);
}

// the volume and the structure count of a structure-report call (structure_kernels.hip): every extent >= min_dim (2 where det J
// reads a neighbour, else 1), fewer than 2^30 voxels, K structures in 1 .. IRS_MAX_LABELS
inline bool structure_shape_ok(const char* who, int D, int H, int W, int min_dim, int K) {
    if (D < min_dim || H < min_dim || W < min_dim)
        return !fail("%s: dims (%d, %d, %d), every one >= %d needed", who, D, H, W, min_dim);
    if ((int64_t)D * H * W >= ((int64_t)1 << 30)) return !fail("%s: the volume must have fewer than 2^30 voxels", who);
    return (K >= 1 && K <= IRS_MAX_LABELS) || !fail("%s: K = %d structures, 1..%d", who, K, IRS_MAX_LABELS);
}

// `count` host doubles, every one finite and, with `increasing`, each above the one before (truth_kernels.hip: bin edges, levels)
inline bool thresholds_ok(const char* who, const char* name, const double* values, int count, bool increasing) {
    for (int e = 0; e < count; ++e) {
        if (!isfinite(values[e])) return !fail("%s: %s[%d] = %g is not finite", who, name, e, values[e]);
        if (increasing && e > 0 && !(values[e] > values[e - 1]))
            return !fail("%s: %s[%d] = %g is not above %s[%d] = %g", who, name, e, values[e], name, e - 1, values[e - 1]);
    }
    return true;
}

// a bin or level count within its cap
inline bool count_ok(const char* who, const char* name, int value, int cap) {
    return (value >= 1 && value <= cap) || !fail("%s: %s = %d, 1..%d", who, name, value, cap);
}

// the bins and the two intensity ranges of the MI data term (mi_kernels.hip) -> bn: the fixed bin width in fp32 as hist_bin takes
// it, the moving scale (bins - 3) / (m_hi - m_lo) in double
inline bool mi_bins_ok(const char* who, int bins, float f_lo, float f_hi, float m_lo, float m_hi, MiBins& bn) {
    if (bins < IRS_MI_MIN_BINS || bins > IRS_MI_MAX_BINS) return !fail("%s: bins = %d, %d..%d", who, bins, IRS_MI_MIN_BINS, IRS_MI_MAX_BINS);
    const float lo[2] = {f_lo, m_lo}, hi[2] = {f_hi, m_hi};
    for (int k = 0; k < 2; ++k) {
        const char* name = k == 0 ? "fixed" : "moving";
        if (!isfinite(lo[k]) || !isfinite(hi[k]) || !(hi[k] > lo[k]))
            return !fail("%s: %s range [%g, %g], finite bounds with hi > lo needed", who, name, (double)lo[k], (double)hi[k]);
        const float inv = (float)bins / (hi[k] - lo[k]);  // fp32, as the bin rule states it
        if (!isfinite(inv) || !(inv > 0.0f))
            return !fail("%s: %s range [%g, %g] is too wide or too narrow for float32 bins", who, name, (double)lo[k], (double)hi[k]);
    }
    bn.bins = bins;
    bn.f_lo = f_lo, bn.f_hi = f_hi, bn.f_inv = (float)bins / (f_hi - f_lo);
    bn.m_lo = (double)m_lo;
    bn.m_scale = (double)(bins - 3) / ((double)m_hi - (double)m_lo);
    return true;
}

inline SplineTaps make_spline(int cps) {
    // sampled cubic B-spline (utils/transformation.py:79-102); evaluated in double, stored as float like the reference
    SplineTaps t;
    memset(&t, 0, sizeof(t));
    t.cps = cps;
    const int n = 4 * cps - 1, r = n / 2;
    for (int i = 0; i < n; ++i) {
        const double x = fabs((double)(i - r) / (double)cps);
        double v = 0.0;
        if (x < 1.0) v = 2.0 / 3.0 + (0.5 * x - 1.0) * x * x;
        else if (x < 2.0) v = -1.0 * ((x - 2.0) * (x - 2.0) * (x - 2.0)) / 6.0;
        t.k[i] = (float)v;
    }
    return t;
}

inline int control_points(int n, int cps) { return (int)ceil((double)(n - 1) / (double)cps) + 1 + 2; }  // utils/util.py:61-69

}  // namespace irs
