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
