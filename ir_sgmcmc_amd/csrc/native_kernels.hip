// Native-resolution outputs: the sampled transformation carried from the registration grid back to the image's own voxel grid
// (absent in the reference, whose outputs all live on the registration grid).
//
// The data set pads the native volume n = (n0, n1, n2) by p_a voxels on both sides of axis a (P_a = n_a + 2 p_a) and resizes the
// padded volume to the registration grid m with align_corners, so native index i_a sits at grid coordinate
// (i_a + p_a) (m_a - 1) / (P_a - 1) and a normalised displacement u_a is u_a (P_a - 1) / 2 padded native voxels.  The output is
// grid_sample(border, align_corners) of the PADDED native volume at identity + the displacement resized from m to P, cropped to
// the native box; the pad holds `fill` for the image and 0 for the segmentation and the mask.
//
// One launch, one thread per native voxel, x (the last axis) fastest: every store is coalesced.  Per voxel
//   1. the three channels of u are interpolated trilinearly at the grid coordinate (one set of taps and weights for the three);
//   2. the source position in the padded frame is r_a = (i_a + p_a) + u_a (P_a - 1) / 2 -- one product and one sum, no round trip
//      through normalised coordinates: u = 0 gives r = i + p exactly and the moving volume comes back bit for bit;
//   3. r_a is clamped to [0, P_a - 1], the border rule of the padded volume;
//   4. the taps are read from the UNPADDED volume: a tap outside the native box reads the fill value (every address is clamped
//      into the box first, the fill is a select).  Nearest rounds half to even, as irs_warp_nearest_*.
// Neither the padded copies nor the 3 P^3 up-sampled field exist.  The kernel is templated on the set of outputs; the field
// taps of neighbouring native voxels mostly coincide (the grid is coarser than the image) and are left to the caches.
#include <array>
#include <utility>

#include "kernels.h"

namespace irs {
namespace {

enum : int { kNatIm = 1, kNatSeg = 2, kNatMask = 4, kNatDisp = 8 };

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

template <int OUT>
__global__ __launch_bounds__(kBlock) void native_warp_kernel(const float* __restrict__ u, const float* __restrict__ im,
                                                             const int16_t* __restrict__ seg, const uint8_t* __restrict__ mask,
                                                             int64_t moving_stride, float* __restrict__ im_out,
                                                             int16_t* __restrict__ seg_out, uint8_t* __restrict__ mask_out,
                                                             float* __restrict__ disp_out, NativeGeom gm, Vol vol) {
    IRS_VOXEL(vol, chain, x, y, z, vox);
    const int idx[3] = {z, y, x};  // axis order (D, H, W); channel c of a field belongs to axis 2 - c

    // 1. the displacement at the grid coordinate of this voxel
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
    float uc[3];
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
    if (OUT & kNatDisp) {
#pragma unroll
        for (int c = 0; c < 3; ++c) disp_out[((int64_t)chain * 3 + c) * vol.V + vox] = __fmul_rn(uc[c], gm.out_scale[c]);
    }
    if (!(OUT & (kNatIm | kNatSeg | kNatMask))) return;

    // 2., 3. the source position in the padded frame, clamped to the padded box
    float r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float last = (float)(gm.P[a] - 1);
        const float raw = __fadd_rn((float)(idx[a] + gm.p[a]), __fmul_rn(uc[2 - a], gm.half_extent[a]));
        r[a] = fminf(fmaxf(raw, 0.0f), last);  // a NaN displacement samples the first plane (fmaxf drops it)
    }
    const unsigned nhw = (unsigned)(vol.H * vol.W), nw = (unsigned)vol.W;
    const int64_t mov = (int64_t)chain * moving_stride, outb = (int64_t)chain * vol.V + vox;

    // 4. the taps, read from the unpadded volume
    if (OUT & kNatIm) {
        unsigned off[3][2];
        bool in[3][2];
        float w[3][2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const NativeTap t = native_tap(r[a], gm.P[a] - 1);
            const unsigned stride = a == 0 ? nhw : (a == 1 ? nw : 1u);
            const BoxIndex b0 = box_index(t.i0, gm.p[a], gm.n[a]), b1 = box_index(t.i1, gm.p[a], gm.n[a]);
            off[a][0] = (unsigned)b0.i * stride;
            off[a][1] = (unsigned)b1.i * stride;
            in[a][0] = b0.in;
            in[a][1] = b1.in;
            w[a][0] = t.w0;
            w[a][1] = t.w1;
        }
        const float* src = im + mov;
        float acc = 0.0f;
#pragma unroll
        for (int cz = 0; cz < 2; ++cz)
#pragma unroll
            for (int cy = 0; cy < 2; ++cy)
#pragma unroll
                for (int cx = 0; cx < 2; ++cx) {
                    const float v = src[off[0][cz] + off[1][cy] + off[2][cx]];
                    const float val = (in[0][cz] && in[1][cy] && in[2][cx]) ? v : gm.fill;
                    acc = __fadd_rn(acc, __fmul_rn(val, __fmul_rn(__fmul_rn(w[2][cx], w[1][cy]), w[0][cz])));
                }
        im_out[outb] = acc;
    }
    if (OUT & (kNatSeg | kNatMask)) {
        unsigned off = 0;
        bool in = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const BoxIndex b = box_index((int)nearbyintf(r[a]), gm.p[a], gm.n[a]);
            off += (unsigned)b.i * (a == 0 ? nhw : (a == 1 ? nw : 1u));
            in = in && b.in;
        }
        if (OUT & kNatSeg) seg_out[outb] = in ? seg[mov + off] : (int16_t)0;
        if (OUT & kNatMask) mask_out[outb] = in ? mask[mov + off] : (uint8_t)0;
    }
}

using NativeKernel = void (*)(const float*, const float*, const int16_t*, const uint8_t*, int64_t, float*, int16_t*, uint8_t*,
                              float*, NativeGeom, Vol);

template <int... OUT>
constexpr auto native_kernel_table(std::integer_sequence<int, OUT...>) {
    return std::array<NativeKernel, sizeof...(OUT)>{native_warp_kernel<OUT>...};
}

}  // namespace

void launch_native_warp(const float* u, const float* im, const int16_t* seg, const uint8_t* mask, int64_t moving_stride,
                        float* im_out, int16_t* seg_out, uint8_t* mask_out, float* disp_out, const NativeGeom& gm, int C,
                        hipStream_t st) {
    static constexpr auto table = native_kernel_table(std::make_integer_sequence<int, 16>{});
    const int out = (im_out ? kNatIm : 0) | (seg_out ? kNatSeg : 0) | (mask_out ? kNatMask : 0) | (disp_out ? kNatDisp : 0);
    const Vol vol = make_vol(gm.n[0], gm.n[1], gm.n[2]);
    hipLaunchKernelGGL(table[out], vox_grid(vol, C), dim3(kBlock), 0, st, u, im, seg, mask, moving_stride, im_out, seg_out,
                       mask_out, disp_out, gm, vol);
}

}  // namespace irs
