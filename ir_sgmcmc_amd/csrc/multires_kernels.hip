// Multi-resolution operators of the coarse-to-fine chain start (absent in the reference, which starts every chain on the full
// grid; DESIGN.md section 6, "Coarse-to-fine start"): an image and a mask carried down to a coarser grid, a field carried up to
// a finer one.  The grids are align_corners: along one axis coarse index i of n sits at fine coordinate x_i = i (N - 1) / (n - 1)
// and fine index I at coarse coordinate I (n - 1) / (N - 1), both formed in double as one exact product and one division.
//
// One launch per operator, one thread per OUTPUT element, x (the last axis) fastest: every store is coalesced and no thread
// writes anything but its own element.  The sums are double, taken in a fixed tap order (z, then y, then x), and rounded to
// float once.  The operators run once per level and per run: the per-tap weights are recomputed where they are used, nothing is
// staged, nothing is tuned.
#include "kernels.h"

namespace irs {
namespace {

struct Axis3 {
    int n[3];  // the INPUT extents (D, H, W order)
    int m[3];  // the OUTPUT extents
};

// ---- restriction: the tent filter of half-width r = max(1, (N - 1) / (n - 1)) around x_i, replicate padding
struct Tent {
    double x, r, sum;
    int lo, hi;  // the integers k that may satisfy |k - x| < r lie in [lo, hi]
};
__device__ __forceinline__ double tent_weight(const Tent& t, int k) {
    const double a = fabs((double)k - t.x);
    return a < t.r ? 1.0 - a / t.r : 0.0;
}
__device__ __forceinline__ Tent make_tent(int i, int N, int n) {
    Tent t;
    t.x = (double)((int64_t)i * (N - 1)) / (double)(n - 1);
    t.r = fmax(1.0, (double)(N - 1) / (double)(n - 1));
    t.lo = (int)floor(t.x - t.r) - 1;
    t.hi = (int)ceil(t.x + t.r) + 1;
    t.sum = 0.0;
    for (int k = t.lo; k <= t.hi; ++k) t.sum = __dadd_rn(t.sum, tent_weight(t, k));
    return t;
}

__global__ __launch_bounds__(kBlock) void restrict_image_kernel(const float* __restrict__ im, float* __restrict__ out, Axis3 ax,
                                                                Vol vol) {
    IRS_VOXEL(vol, plane, x, y, z, vox);
    const int N0 = ax.n[0], N1 = ax.n[1], N2 = ax.n[2];
    const Tent tz = make_tent(z, N0, ax.m[0]), ty = make_tent(y, N1, ax.m[1]), tx = make_tent(x, N2, ax.m[2]);
    const float* src = im + (int64_t)plane * N0 * N1 * N2;
    double acc = 0.0;
    for (int kz = tz.lo; kz <= tz.hi; ++kz) {
        const double wz = tent_weight(tz, kz) / tz.sum;
        if (wz == 0.0) continue;  // |kz - x| >= r: no tap
        const int oz = min(max(kz, 0), N0 - 1) * N1;
        for (int ky = ty.lo; ky <= ty.hi; ++ky) {
            const double wy = tent_weight(ty, ky) / ty.sum;
            if (wy == 0.0) continue;
            const int row = (oz + min(max(ky, 0), N1 - 1)) * N2;
            const double wzy = __dmul_rn(wz, wy);
            for (int kx = tx.lo; kx <= tx.hi; ++kx) {
                const double wx = tent_weight(tx, kx) / tx.sum;
                if (wx == 0.0) continue;
                const double v = (double)src[row + min(max(kx, 0), N2 - 1)];
                acc = __dadd_rn(acc, __dmul_rn(__dmul_rn(wzy, wx), v));
            }
        }
    }
    out[(int64_t)plane * vol.V + vox] = (float)acc;
}

// the coarse voxel takes the fine voxel at floor(x_i + 0.5) per axis
__device__ __forceinline__ int nearest_fine(int i, int N, int n) {
    const double x = (double)((int64_t)i * (N - 1)) / (double)(n - 1);
    return min((int)floor(x + 0.5), N - 1);
}

__global__ __launch_bounds__(kBlock) void restrict_mask_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, Axis3 ax,
                                                               Vol vol) {
    IRS_VOXEL(vol, plane, x, y, z, vox);
    const int kz = nearest_fine(z, ax.n[0], ax.m[0]), ky = nearest_fine(y, ax.n[1], ax.m[1]), kx = nearest_fine(x, ax.n[2], ax.m[2]);
    const int64_t Vin = (int64_t)ax.n[0] * ax.n[1] * ax.n[2];
    out[(int64_t)plane * vol.V + vox] = mask[plane * Vin + ((int64_t)kz * ax.n[1] + ky) * ax.n[2] + kx];
}

// ---- prolongation: trilinear at the coarse coordinate of the fine voxel; the values are not rescaled
struct Lerp {
    int i0;
    bool two;  // the upper tap i0 + 1 exists (< n); where it does not, its weight is 0 and it is not read
    double w[2];
};
__device__ __forceinline__ Lerp make_lerp(int I, int n, int N) {
    Lerp t;
    const double c = (double)((int64_t)I * (n - 1)) / (double)(N - 1);
    t.i0 = min((int)floor(c), n - 1);
    t.two = t.i0 + 1 < n;
    t.w[1] = c - (double)t.i0;
    t.w[0] = 1.0 - t.w[1];
    return t;
}

__global__ __launch_bounds__(kBlock) void prolong_field_kernel(const float* __restrict__ in, float* __restrict__ out, Axis3 ax,
                                                               Vol vol) {
    IRS_VOXEL(vol, plane, x, y, z, vox);
    const int n1 = ax.n[1], n2 = ax.n[2];
    const Lerp tz = make_lerp(z, ax.n[0], ax.m[0]), ty = make_lerp(y, n1, ax.m[1]), tx = make_lerp(x, n2, ax.m[2]);
    const float* src = in + (int64_t)plane * ax.n[0] * n1 * n2;
    double acc = 0.0;
#pragma unroll
    for (int cz = 0; cz < 2; ++cz) {
        if (cz && !tz.two) continue;
#pragma unroll
        for (int cy = 0; cy < 2; ++cy) {
            if (cy && !ty.two) continue;
            const int row = ((tz.i0 + cz) * n1 + ty.i0 + cy) * n2;
            const double wzy = __dmul_rn(tz.w[cz], ty.w[cy]);
#pragma unroll
            for (int cx = 0; cx < 2; ++cx) {
                if (cx && !tx.two) continue;
                acc = __dadd_rn(acc, __dmul_rn(__dmul_rn(wzy, tx.w[cx]), (double)src[row + tx.i0 + cx]));
            }
        }
    }
    out[(int64_t)plane * vol.V + vox] = (float)acc;
}

Axis3 axes(const Vol& in, const Vol& out) { return Axis3{{in.D, in.H, in.W}, {out.D, out.H, out.W}}; }

}  // namespace

void launch_restrict_image(const float* im, float* out, int planes, const Vol& fine, const Vol& coarse, hipStream_t st) {
    hipLaunchKernelGGL(restrict_image_kernel, vox_grid(coarse, planes), dim3(kBlock), 0, st, im, out, axes(fine, coarse), coarse);
}

void launch_restrict_mask(const uint8_t* mask, uint8_t* out, int planes, const Vol& fine, const Vol& coarse, hipStream_t st) {
    hipLaunchKernelGGL(restrict_mask_kernel, vox_grid(coarse, planes), dim3(kBlock), 0, st, mask, out, axes(fine, coarse), coarse);
}

void launch_prolong_field(const float* in, float* out, int planes, const Vol& coarse, const Vol& fine, hipStream_t st) {
    hipLaunchKernelGGL(prolong_field_kernel, vox_grid(fine, planes), dim3(kBlock), 0, st, in, out, axes(coarse, fine), fine);
}

}  // namespace irs
