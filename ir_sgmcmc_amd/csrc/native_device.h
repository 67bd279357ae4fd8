// Device helpers of the native-resolution warps, shared by native_kernels.hip (irs_native_warp) and bspline_kernels.hip
// (irs_native_warp_cubic): the steps that lead from a native voxel to its source position in the padded frame, and the
// trilinear blend of the unpadded image with the fill.  Every operation is an explicit round-to-nearest intrinsic, so the two
// kernels compute the same bits from the same inputs whatever the compiler makes of the code around them.
#pragma once
#include "kernels.h"

namespace irs {

// tap pair and weights of one axis at the position r, 0 <= r <= last
struct NativeTap {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ NativeTap native_tap(float r, int last) {
    NativeTap t;
    const float f = floorf(r);
    t.i0 = min((int)f, last);
    t.i1 = min(t.i0 + 1, last);
    t.w1 = __fsub_rn(r, f);
    t.w0 = __fsub_rn(__fadd_rn(f, 1.0f), r);
    return t;
}

// one axis of the moving volume: the padded index k (0 <= k < P) as an index clamped into the native box and whether it was in it
struct BoxIndex {
    int i;
    bool in;
};
__device__ __forceinline__ BoxIndex box_index(int k, int p, int n) {
    const int i = k - p;
    return {min(max(i, 0), n - 1), i >= 0 && i < n};
}

// step 1: the three channels of the displacement u (C,3,m) at the grid coordinate of native voxel idx = (z, y, x)
__device__ __forceinline__ void native_displacement(const float* __restrict__ u, int chain, const int (&idx)[3], const NativeGeom& gm,
                                                    float (&uc)[3]) {
    NativeTap ft[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float g = fminf(__fmul_rn((float)(idx[a] + gm.p[a]), gm.grid_step[a]), (float)(gm.m[a] - 1));
        ft[a] = native_tap(g, gm.m[a] - 1);
    }
    const unsigned mhw = (unsigned)(gm.m[1] * gm.m[2]), mw = (unsigned)gm.m[2];
    const unsigned fz[2] = {(unsigned)ft[0].i0 * mhw, (unsigned)ft[0].i1 * mhw};
    const unsigned fy[2] = {(unsigned)ft[1].i0 * mw, (unsigned)ft[1].i1 * mw};
    const unsigned fx[2] = {(unsigned)ft[2].i0, (unsigned)ft[2].i1};
    const int64_t Vm = (int64_t)gm.m[0] * gm.m[1] * gm.m[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* f = u + ((int64_t)chain * 3 + c) * Vm;
        float pz[2];
#pragma unroll
        for (int cz = 0; cz < 2; ++cz) {
            float py[2];
#pragma unroll
            for (int cy = 0; cy < 2; ++cy) {
                const unsigned row = fz[cz] + fy[cy];
                py[cy] = __fadd_rn(__fmul_rn(ft[2].w0, f[row + fx[0]]), __fmul_rn(ft[2].w1, f[row + fx[1]]));
            }
            pz[cz] = __fadd_rn(__fmul_rn(ft[1].w0, py[0]), __fmul_rn(ft[1].w1, py[1]));
        }
        uc[c] = __fadd_rn(__fmul_rn(ft[0].w0, pz[0]), __fmul_rn(ft[0].w1, pz[1]));
    }
}

// steps 2 and 3: the source position in the padded frame, clamped to the padded box (axis order; channel c belongs to axis 2 - c)
__device__ __forceinline__ void native_source(const float (&uc)[3], const int (&idx)[3], const NativeGeom& gm, float (&r)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float last = (float)(gm.P[a] - 1);
        const float raw = __fadd_rn((float)(idx[a] + gm.p[a]), __fmul_rn(uc[2 - a], gm.half_extent[a]));
        r[a] = fminf(fmaxf(raw, 0.0f), last);  // a NaN displacement samples the first plane (fmaxf drops it)
    }
}

// the eight trilinear taps of r in the unpadded volume: offsets clamped into the native box, whether each tap lay in it, weights
struct NativeTaps {
    unsigned off[3][2];
    bool in[3][2];
    float w[3][2];
};
__device__ __forceinline__ NativeTaps native_taps(const float (&r)[3], const NativeGeom& gm) {
    NativeTaps nt;
    const unsigned nhw = (unsigned)(gm.n[1] * gm.n[2]), nw = (unsigned)gm.n[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const NativeTap t = native_tap(r[a], gm.P[a] - 1);
        const unsigned stride = a == 0 ? nhw : (a == 1 ? nw : 1u);
        const BoxIndex b0 = box_index(t.i0, gm.p[a], gm.n[a]), b1 = box_index(t.i1, gm.p[a], gm.n[a]);
        nt.off[a][0] = (unsigned)b0.i * stride;
        nt.off[a][1] = (unsigned)b1.i * stride;
        nt.in[a][0] = b0.in;
        nt.in[a][1] = b1.in;
        nt.w[a][0] = t.w0;
        nt.w[a][1] = t.w1;
    }
    return nt;
}

// step 4 for the image: the trilinear blend, a tap outside the native box reading the fill
__device__ __forceinline__ float native_trilinear(const float* __restrict__ src, const NativeTaps& nt, float fill) {
    float acc = 0.0f;
#pragma unroll
    for (int cz = 0; cz < 2; ++cz)
#pragma unroll
        for (int cy = 0; cy < 2; ++cy)
#pragma unroll
            for (int cx = 0; cx < 2; ++cx) {
                const float v = src[nt.off[0][cz] + nt.off[1][cy] + nt.off[2][cx]];
                const float val = (nt.in[0][cz] && nt.in[1][cy] && nt.in[2][cx]) ? v : fill;
                acc = __fadd_rn(acc, __fmul_rn(val, __fmul_rn(__fmul_rn(nt.w[2][cx], nt.w[1][cy]), nt.w[0][cz])));
            }
    return acc;
}

}  // namespace irs
