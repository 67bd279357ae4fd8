// Affine pre-alignment (absent in the reference, whose volumes were registered affinely elsewhere; DESIGN.md section 6, "Affine
// pre-alignment"): the Gauss-Newton normal equations of the sum of squared differences under a 3 x 4 map, the map as a
// transformation tensor, and the map composed with a sampled transformation.
//
// Conventions.  Voxel index coordinates in array order (D, H, W): index k = (k0, k1, k2), centre c = ((D - 1) / 2, (H - 1) / 2,
// (W - 1) / 2); fixed and moving volume have the same extents.  A map is lin (3 x 3, row-major) and shift (3), float64, passed by
// value.  Fixed voxel k reads the moving image at p = c + shift + lin (k - c), formed in double, every operation rounded once
// and none contracted:  p_a = ((lin[a][0] d_0 + lin[a][1] d_1) + lin[a][2] d_2 + shift[a]) + c_a  with d = k - c (exact), left to
// right.  The identity gives p = k exactly.
//  - A voxel takes part when the mask is set (or absent), 0 <= p_a <= n_a - 1 on all three axes, and the fixed value and all
//    eight moving taps are finite.  The tests are made in that order: a masked voxel mapped outside is counted as outside and
//    its taps are not read; one inside with a non-finite value is counted as non-finite.
//  - Cell: i0 = min(floor(p), n - 2), w = p - i0 per axis: on an integer coordinate the forward cell, at p = n - 1 the weight 1.
//  - Value: M = sum over the taps in the order z, y, x of ((wz wy) wx) t, the taps t float32 -> double, the weights (1 - w, w).
//    Gradient g = dM/dp in array order, the interpolant's: g_0 = sum over (y, x) of (wy wx) (t[1][y][x] - t[0][y][x]), g_1 = sum
//    over (z, x) of (wz wx) (t[z][1][x] - t[z][0][x]), g_2 = sum over (z, y) of (wz wy) (t[z][y][1] - t[z][y][0]).  r = M - F.
//  - Parameters theta = (lin row-major, shift): with kt = (d_0, d_1, d_2, 1), dr/dlin[a][b] = g_a kt_b and dr/dshift[a] =
//    g_a kt_3.  H = sum J J^T is accumulated as its 60 distinct sums S[(i,j)][(a,b)] = sum (g_i g_j) (kt_a kt_b), i <= j, a <= b;
//    b = sum J r as the 12 sums (g_a r) kt_b; then sum r^2 and the three counts (doubles: exact below 2^53).
//
// Two launches.  accumulate: the row walk of the reduction kernels (a wavefront per row (y, z), its lanes along x); every thread
// keeps the 76 sums in registers as doubles, the block folds them with block_sum in four groups of 19 and writes ONE row of
// partials.  One pass at low occupancy rather than two passes over the gather: 76 doubles are 152 VGPRs before any temporary,
// and the kernel compiles to 256 VGPRs + 112 AGPRs without scratch, one wavefront per SIMD (512 registers per lane, granule 8:
// above 256 -> 1).  Capped at two wavefronts per SIMD it spills 448 bytes per lane, which is refused; a pass that holds the 60
// sums alone would still gather and interpolate everything a second time.  The stage is some tens of launches per run
// (DESIGN.md has the measurements).  finish: one block; thread i takes row i of the partials, the block folds them with
// the same block_sum (a fixed order), then the 94 outputs are expanded.  No floating-point atomics, a grid that depends on the
// extents only: two identical calls are bit-identical.
#include <algorithm>

#include "kernels.h"

namespace irs {
namespace {

constexpr int kGG = 6, kKK = 10, kS = kGG * kKK;  // 60
constexpr int kB = 12;
constexpr int kCols = IRS_AFFINE_PARTIALS;  // 60 + 12 + sum r^2 + three counts
static_assert(kCols == kS + kB + 4, "layout of a row of partials");
static_assert(IRS_AFFINE_SUMS == 78 + 12 + 4, "layout of the sums");
constexpr int kGroup = 19, kGroups = kCols / kGroup;
static_assert(kGroup * kGroups == kCols, "the block reduction takes the columns in equal groups");

// index of the unordered pair (i, j) of 0 .. n - 1 in the row-major upper triangle
__host__ __device__ constexpr int sym(int i, int j, int n) {
    return i <= j ? i * n - i * (i - 1) / 2 + (j - i) : j * n - j * (j - 1) / 2 + (i - j);
}

struct Cell {
    int i0;
    double w[2];
};
__device__ __forceinline__ Cell make_cell(double p, int n) {
    Cell c;
    c.i0 = min((int)floor(p), n - 2);
    c.w[1] = __dsub_rn(p, (double)c.i0);
    c.w[0] = __dsub_rn(1.0, c.w[1]);
    return c;
}

// p_a of the header comment
__device__ __forceinline__ double map_axis(const double* lin, double shift, double c, double d0, double d1, double d2) {
    const double dot = __dadd_rn(__dadd_rn(__dmul_rn(lin[0], d0), __dmul_rn(lin[1], d1)), __dmul_rn(lin[2], d2));
    return __dadd_rn(__dadd_rn(dot, shift), c);
}

__global__ __launch_bounds__(kBlock) void affine_accumulate_kernel(const float* __restrict__ fixed, const float* __restrict__ moving,
                                                                   const uint8_t* __restrict__ mask, Vol vol, AffineMap map,
                                                                   double* __restrict__ partials) {
    __shared__ double smem[kCols * (kBlock / kWave)];
    double s[kCols];
#pragma unroll
    for (int j = 0; j < kCols; ++j) s[j] = 0.0;
    const int n0 = vol.D, n1 = vol.H, n2 = vol.W;
    const double c0 = 0.5 * (double)(n0 - 1), c1 = 0.5 * (double)(n1 - 1), c2 = 0.5 * (double)(n2 - 1);

    IRS_ROWS_BEGIN(vol, x, y, z, vox)
    if (mask && mask[vox] == 0) continue;
    double kt[4] = {(double)z - c0, (double)y - c1, (double)x - c2, 1.0};
    const double p0 = map_axis(map.lin + 0, map.shift[0], c0, kt[0], kt[1], kt[2]);
    const double p1 = map_axis(map.lin + 3, map.shift[1], c1, kt[0], kt[1], kt[2]);
    const double p2 = map_axis(map.lin + 6, map.shift[2], c2, kt[0], kt[1], kt[2]);
    if (!(p0 >= 0.0 && p0 <= (double)(n0 - 1) && p1 >= 0.0 && p1 <= (double)(n1 - 1) && p2 >= 0.0 && p2 <= (double)(n2 - 1))) {
        s[kS + kB + 2] += 1.0;
        continue;
    }
    const Cell cz = make_cell(p0, n0), cy = make_cell(p1, n1), cx = make_cell(p2, n2);
    const float f = fixed[vox];
    float tf[2][2][2];
    bool finite = isfinite(f);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                tf[a][b][c] = moving[((int64_t)(cz.i0 + a) * n1 + (cy.i0 + b)) * n2 + (cx.i0 + c)];
                finite = finite && isfinite(tf[a][b][c]);
            }
    if (!finite) {
        s[kS + kB + 3] += 1.0;
        continue;
    }
    double t[2][2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c) t[a][b][c] = (double)tf[a][b][c];

    double m = 0.0, g[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const double wzy = __dmul_rn(cz.w[a], cy.w[b]);
#pragma unroll
            for (int c = 0; c < 2; ++c) m = __dadd_rn(m, __dmul_rn(__dmul_rn(wzy, cx.w[c]), t[a][b][c]));
            // a, b as the two axes that are not differentiated, in array order
            g[0] = __dadd_rn(g[0], __dmul_rn(__dmul_rn(cy.w[a], cx.w[b]), __dsub_rn(t[1][a][b], t[0][a][b])));
            g[1] = __dadd_rn(g[1], __dmul_rn(__dmul_rn(cz.w[a], cx.w[b]), __dsub_rn(t[a][1][b], t[a][0][b])));
            g[2] = __dadd_rn(g[2], __dmul_rn(wzy, __dsub_rn(t[a][b][1], t[a][b][0])));
        }
    const double r = __dsub_rn(m, (double)f);

    double kk[kKK];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) kk[sym(a, b, 4)] = __dmul_rn(kt[a], kt[b]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double gg = __dmul_rn(g[i], g[j]);
#pragma unroll
            for (int q = 0; q < kKK; ++q) s[sym(i, j, 3) * kKK + q] = __dadd_rn(s[sym(i, j, 3) * kKK + q], __dmul_rn(gg, kk[q]));
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double gr = __dmul_rn(g[a], r);
#pragma unroll
        for (int b = 0; b < 4; ++b) s[kS + a * 4 + b] = __dadd_rn(s[kS + a * 4 + b], __dmul_rn(gr, kt[b]));
    }
    s[kS + kB] = __dadd_rn(s[kS + kB], __dmul_rn(r, r));
    s[kS + kB + 1] += 1.0;
    IRS_ROWS_END

    // in groups: block_sum holds a second copy of what it folds
#pragma unroll
    for (int q = 0; q < kGroups; ++q) {
        double v[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) v[j] = s[q * kGroup + j];
        block_sum<kGroup>(v, smem + q * kGroup * (kBlock / kWave));
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < kGroup; ++j) partials[(int64_t)blockIdx.x * kCols + q * kGroup + j] = v[j];
        }
    }
}

constexpr int kFinishThreads = IRS_AFFINE_MAX_BLOCKS;
static_assert(kFinishThreads <= 1024 && kFinishThreads % kWave == 0 && kFinishThreads >= IRS_AFFINE_SUMS,
              "the finish kernel folds one row of partials per thread, then writes one output per thread");

// parameter index -> (row of lin / entry of shift = which g, which kt)
__device__ __forceinline__ void param_axes(int p, int& gi, int& ki) {
    gi = p < 9 ? p / 3 : p - 9;
    ki = p < 9 ? p - 3 * gi : 3;
}

__global__ __launch_bounds__(kFinishThreads) void affine_finish_kernel(const double* __restrict__ partials, int nblocks,
                                                                       double* __restrict__ sums) {
    constexpr int G = kFinishThreads / kWave;
    __shared__ double smem[kCols * G];
    __shared__ double col[kCols];
    const int j = threadIdx.x;
    // thread i takes row i (a serial walk down a column is a thousand dependent L2 round trips); then as in a block: the lanes by
    // the shuffle butterfly, the wavefronts in order
#pragma unroll
    for (int q = 0; q < kGroups; ++q) {
        double v[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) v[i] = j < nblocks ? partials[(int64_t)j * kCols + q * kGroup + i] : 0.0;
        block_sum<kGroup, G>(v, smem + q * kGroup * G);
        if (j == 0) {
#pragma unroll
            for (int i = 0; i < kGroup; ++i) col[q * kGroup + i] = v[i];
        }
    }
    __syncthreads();
    if (j < 78) {
        // entry j of the row-major upper triangle of the 12 x 12 matrix -> (p, q), p <= q
        int p = 0, left = j;
        while (left >= 12 - p) {
            left -= 12 - p;
            ++p;
        }
        const int q = p + left;
        int gp, kp, gq, kq;
        param_axes(p, gp, kp);
        param_axes(q, gq, kq);
        sums[j] = col[sym(gp, gq, 3) * kKK + sym(kp, kq, 4)];
    } else if (j < 90) {
        int gp, kp;
        param_axes(j - 78, gp, kp);
        sums[j] = col[kS + gp * 4 + kp];
    } else if (j < IRS_AFFINE_SUMS) {
        sums[j] = col[kS + kB + (j - 90)];
    }
}

// the [-1, 1] coordinate of index coordinate p on an axis of n nodes (align_corners), in double
__device__ __forceinline__ double to_normalised(double p, int n) { return __dsub_rn(__ddiv_rn(__dmul_rn(2.0, p), (double)(n - 1)), 1.0); }

__global__ __launch_bounds__(kBlock) void affine_transformation_kernel(float* __restrict__ out, AffineMap map, Vol vol) {
    IRS_VOXEL(vol, plane, x, y, z, vox);
    (void)plane;
    const double c0 = 0.5 * (double)(vol.D - 1), c1 = 0.5 * (double)(vol.H - 1), c2 = 0.5 * (double)(vol.W - 1);
    const double d0 = (double)z - c0, d1 = (double)y - c1, d2 = (double)x - c2;
    out[vox] = (float)to_normalised(map_axis(map.lin + 6, map.shift[2], c2, d0, d1, d2), vol.W);
    out[vol.V + vox] = (float)to_normalised(map_axis(map.lin + 3, map.shift[1], c1, d0, d1, d2), vol.H);
    out[2 * vol.V + vox] = (float)to_normalised(map_axis(map.lin + 0, map.shift[0], c0, d0, d1, d2), vol.D);
}

// the index coordinate of [-1, 1] coordinate g, the expression of the warps in double: ((g + 1) / 2) (n - 1); not clamped
__device__ __forceinline__ double to_index(float g, int n) { return __dmul_rn(__dmul_rn(__dadd_rn((double)g, 1.0), 0.5), (double)(n - 1)); }

__global__ __launch_bounds__(kBlock) void affine_compose_kernel(const float* __restrict__ transformation, AffineMap map,
                                                                float* __restrict__ total_t, float* __restrict__ total_d, Vol vol) {
    IRS_VOXEL(vol, chain, x, y, z, vox);
    const int64_t base = (int64_t)chain * 3 * vol.V + vox;
    const double c0 = 0.5 * (double)(vol.D - 1), c1 = 0.5 * (double)(vol.H - 1), c2 = 0.5 * (double)(vol.W - 1);
    const double d0 = __dsub_rn(to_index(transformation[base + 2 * vol.V], vol.D), c0);
    const double d1 = __dsub_rn(to_index(transformation[base + vol.V], vol.H), c1);
    const double d2 = __dsub_rn(to_index(transformation[base], vol.W), c2);
    const double q0 = map_axis(map.lin + 0, map.shift[0], c0, d0, d1, d2);
    const double q1 = map_axis(map.lin + 3, map.shift[1], c1, d0, d1, d2);
    const double q2 = map_axis(map.lin + 6, map.shift[2], c2, d0, d1, d2);
    if (total_t) {
        total_t[base] = (float)to_normalised(q2, vol.W);
        total_t[base + vol.V] = (float)to_normalised(q1, vol.H);
        total_t[base + 2 * vol.V] = (float)to_normalised(q0, vol.D);
    }
    if (total_d) {
        total_d[base] = (float)__dsub_rn(q2, (double)x);
        total_d[base + vol.V] = (float)__dsub_rn(q1, (double)y);
        total_d[base + 2 * vol.V] = (float)__dsub_rn(q0, (double)z);
    }
}

}  // namespace

// rows of partials = blocks: depends on the extents only
static int affine_blocks(const Vol& vol) {
    const int64_t rows = (int64_t)vol.H * vol.D, per_block = kBlock / kWave;
    return (int)std::max<int64_t>(1, std::min<int64_t>((rows + per_block - 1) / per_block, IRS_AFFINE_MAX_BLOCKS));
}

void launch_affine_normal_equations(const float* fixed, const float* moving, const uint8_t* mask, const Vol& vol, const AffineMap& map,
                                    double* sums, double* partials, hipStream_t st) {
    const int blocks = affine_blocks(vol);
    hipLaunchKernelGGL(affine_accumulate_kernel, dim3(blocks), dim3(kBlock), 0, st, fixed, moving, mask, vol, map, partials);
    hipLaunchKernelGGL(affine_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, partials, blocks, sums);
}

void launch_affine_transformation(const AffineMap& map, float* out, const Vol& vol, hipStream_t st) {
    hipLaunchKernelGGL(affine_transformation_kernel, vox_grid(vol, 1), dim3(kBlock), 0, st, out, map, vol);
}

void launch_affine_compose(const float* transformation, const AffineMap& map, float* total_transformation, float* total_displacement,
                           int C, const Vol& vol, hipStream_t st) {
    hipLaunchKernelGGL(affine_compose_kernel, vox_grid(vol, C), dim3(kBlock), 0, st, transformation, map, total_transformation,
                       total_displacement, vol);
}

}  // namespace irs
