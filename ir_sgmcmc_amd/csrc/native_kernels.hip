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

#include "native_device.h"

namespace irs {
namespace {

enum : int { kNatIm = 1, kNatSeg = 2, kNatMask = 4, kNatDisp = 8 };

template <int OUT>
__global__ __launch_bounds__(kBlock) void native_warp_kernel(const float* __restrict__ u, const float* __restrict__ im,
                                                             const int16_t* __restrict__ seg, const uint8_t* __restrict__ mask,
                                                             int64_t moving_stride, float* __restrict__ im_out,
                                                             int16_t* __restrict__ seg_out, uint8_t* __restrict__ mask_out,
                                                             float* __restrict__ disp_out, NativeGeom gm, Vol vol) {
    IRS_VOXEL(vol, chain, x, y, z, vox);
    const int idx[3] = {z, y, x};  // axis order (D, H, W); channel c of a field belongs to axis 2 - c

    // 1. the displacement at the grid coordinate of this voxel
    float uc[3];
    native_displacement(u, chain, idx, gm, uc);
    if (OUT & kNatDisp) {
#pragma unroll
        for (int c = 0; c < 3; ++c) disp_out[((int64_t)chain * 3 + c) * vol.V + vox] = __fmul_rn(uc[c], gm.out_scale[c]);
    }
    if (!(OUT & (kNatIm | kNatSeg | kNatMask))) return;

    // 2., 3. the source position in the padded frame, clamped to the padded box
    float r[3];
    native_source(uc, idx, gm, r);
    const unsigned nhw = (unsigned)(vol.H * vol.W), nw = (unsigned)vol.W;
    const int64_t mov = (int64_t)chain * moving_stride, outb = (int64_t)chain * vol.V + vox;

    // 4. the taps, read from the unpadded volume
    if (OUT & kNatIm) im_out[outb] = native_trilinear(im + mov, native_taps(r, gm), gm.fill);
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
