// The LNCC data term (absent in the reference, whose data terms compare intensities voxel by voxel): the
// squared local normalised cross-correlation of VoxelMorph over the (2R+1)^3 box window with clamped indices, and its exact
// adjoint with respect to the moving image.  All of it float32, as include/irsgmcmc.h states it:
//   A = S_fm - S_f S_m / n, Bf = S_ff - S_f^2 / n, Bm = S_mm - S_m^2 / n, den = Bf Bm + eps, d = 1 - A^2 / den
//   p = 2 u A / den, q = 2 u A^2 Bf / den^2, t = (q S_m - p S_f) / n
//   g_M = M box^T(q) - F box^T(p) - box^T(t)
// Both kernels are z-marching column tiles like local_similarity_kernels.hip: a work item is one 32 x 8 tile in x-y over one
// z-segment, a block of 256 threads walks its work items (blockIdx.x, + gridDim.x, ...), one column per thread; blockIdx.y is the
// chain, so every chain runs in the one launch.
//  - forward kernel, per plane of z0 - R .. z1 - 1 + R (clamped: a plane past an end is the end plane again):
//      A  tile + halo R of F and M, indices clamped in x and y, to LDS;
//      B  per element of the tile and its y-halo the five x-sums over 2R+1 neighbours (f, m, f f, m m, f m) to LDS;
//      C  per thread the five y-sums over 2R+1 rows: the plane sums of its column, pushed into the thread's ring of 2R+1 plane
//         sums -- in registers, shifted by one per plane (every index static: no scratch);
//      D  the output plane z = p - R once it is inside the segment: the ring RE-SUMMED from the oldest plane to the newest -- no
//         running z-sum, so nothing non-finite outlives its plane -- then p, q, t, optionally d, and u d into the thread's double.
//    One double of sum u d per workgroup and chain, summed in a fixed order (block_sum), then scaled.
//  - adjoint kernel: box^T is the box over the ZERO-padded coefficient maps with the padding folded back onto the face it was
//    replicated from: the tap at offset k of a voxel on the low face counts R - k times more, on the high face R + k times more
//    (k = -R .. R; what lies outside is zero, so only the taps that exist contribute).  Per plane of z0 - R .. z1 - 1 + R (a plane
//    outside the volume is a plane of zeros): tile + halo of p, q, t to LDS, the folded x-sums to LDS, the folded y-sums into
//    the ring, and per output plane the folded z-sum of the ring, combined with F and M.
// No atomics.  The grid and every order of summation depend on (D, H, W, R) and the segment length only: two identical calls are
// bit-identical and chain c of a batch equals the single-chain call.
#include <algorithm>

#include "kernels.h"

namespace irs {
namespace {

constexpr int kLnTX = 32, kLnTY = 8;  // the tile: one column per thread
static_assert(kLnTX * kLnTY == kBlock, "one thread per column of the tile");

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
// how many times more than once the tap at offset k of the voxel at index i counts: the replicate padding folded back (0 inside)
__device__ __forceinline__ float fold_weight(int i, int n, int k, int R) {
    return (float)(1 + (i == 0 ? R - k : 0) + (i == n - 1 ? R + k : 0));
}

template <int R>
__global__ __launch_bounds__(kBlock) void lncc_fwd_kernel(const float* __restrict__ fixed, int64_t fixed_stride,
                                                          const float* __restrict__ moving, const float* __restrict__ upstream,
                                                          int64_t upstream_stride, const uint8_t* __restrict__ mask,
                                                          int64_t mask_stride, LnccGeom g, float eps, double scale,
                                                          float* __restrict__ d_out, float* __restrict__ coef,
                                                          double* __restrict__ partials) {
    constexpr int NT = 2 * R + 1, HX = kLnTX + 2 * R, HY = kLnTY + 2 * R;
    __shared__ float TF[HY * HX], TM[HY * HX];  // [row][x]
    __shared__ float XS[5 * HY * kLnTX];        // [sum][row][x]
    __shared__ double smem[kBlock / kWave];

    const int chain = blockIdx.y;
    const int64_t V = (int64_t)g.D * g.H * g.W;
    const float* f = fixed + (int64_t)chain * fixed_stride;
    const float* m = moving + (int64_t)chain * V;
    const float* up = upstream ? upstream + (int64_t)chain * upstream_stride : nullptr;
    const uint8_t* mk = mask ? mask + (int64_t)chain * mask_stride : nullptr;
    float* dc = d_out ? d_out + (int64_t)chain * V : nullptr;
    float* cc = coef ? coef + (int64_t)chain * 3 * V : nullptr;
    const int tx = threadIdx.x & (kLnTX - 1), ty = threadIdx.x / kLnTX;
    const float n = (float)(NT * NT * NT);
    double acc[1] = {0.0};

    for (int work = blockIdx.x; work < g.nwork; work += gridDim.x) {
        const int seg = work / g.tiles, tile = work - seg * g.tiles;
        const int x0 = (tile % g.tiles_x) * kLnTX, y0 = (tile / g.tiles_x) * kLnTY;
        const int z0 = seg * g.seg_len, z1 = min(z0 + g.seg_len, g.D);
        const int x = x0 + tx, y = y0 + ty;
        const bool inside = x < g.W && y < g.H;
        float ring[5][NT];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int t = 0; t < NT; ++t) ring[q][t] = 0.0f;
        for (int p = z0 - R; p < z1 + R; ++p) {
            const int plane = clampi(p, g.D - 1) * g.H;
            __syncthreads();  // the tiles and XS of the plane before have been read
            for (int i = threadIdx.x; i < HX * HY; i += kBlock) {
                const int hy = i / HX, hx = i - hy * HX;
                const int src = (plane + clampi(y0 + hy - R, g.H - 1)) * g.W + clampi(x0 + hx - R, g.W - 1);
                TF[i] = f[src];
                TM[i] = m[src];
            }
            __syncthreads();
            for (int i = threadIdx.x; i < kLnTX * HY; i += kBlock) {
                const int hy = i / kLnTX, xx = i - hy * kLnTX;
                float sf = 0.0f, sm = 0.0f, sff = 0.0f, smm = 0.0f, sfm = 0.0f;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float vf = TF[hy * HX + xx + t], vm = TM[hy * HX + xx + t];
                    sf += vf;
                    sm += vm;
                    sff += vf * vf;
                    smm += vm * vm;
                    sfm += vf * vm;
                }
                XS[0 * HY * kLnTX + i] = sf;
                XS[1 * HY * kLnTX + i] = sm;
                XS[2 * HY * kLnTX + i] = sff;
                XS[3 * HY * kLnTX + i] = smm;
                XS[4 * HY * kLnTX + i] = sfm;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                float s = 0.0f;
#pragma unroll
                for (int t = 0; t < NT; ++t) s += XS[(q * HY + ty + t) * kLnTX + tx];
#pragma unroll
                for (int t = 0; t + 1 < NT; ++t) ring[q][t] = ring[q][t + 1];
                ring[q][NT - 1] = s;  // the newest plane last
            }
            const int z = p - R;
            if (z < z0) continue;
            float S[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                float s = 0.0f;
#pragma unroll
                for (int t = 0; t < NT; ++t) s += ring[q][t];
                S[q] = s;
            }
            if (!inside) continue;
            const int v = (z * g.H + y) * g.W + x;
            const float u = up ? up[v] : mk ? (float)mk[v] : 1.0f;
            const float A = S[4] - S[0] * S[1] / n;
            const float Bf = S[2] - S[0] * S[0] / n;
            const float Bm = S[3] - S[1] * S[1] / n;
            const float den = Bf * Bm + eps;
            const float r = A / den;
            const float pc = 2.0f * u * r;
            const float qc = pc * r * Bf;
            const float d = 1.0f - A * r;
            if (cc) {
                cc[v] = pc;
                cc[V + v] = qc;
                cc[2 * V + v] = (qc * S[1] - pc * S[0]) / n;
            }
            if (dc) dc[v] = d;
            acc[0] += (double)u * (double)d;
        }
    }
    if (!partials) return;
    __syncthreads();
    block_sum<1>(acc, smem);
    if (threadIdx.x == 0) partials[(int64_t)chain * gridDim.x + blockIdx.x] = scale * acc[0];
}

template <int R>
__global__ __launch_bounds__(kBlock) void lncc_bwd_kernel(const float* __restrict__ fixed, int64_t fixed_stride,
                                                          const float* __restrict__ moving, const float* __restrict__ coef,
                                                          LnccGeom g, float scale, float* __restrict__ g_moving) {
    constexpr int NT = 2 * R + 1, HX = kLnTX + 2 * R, HY = kLnTY + 2 * R;
    __shared__ float T[3 * HY * HX];      // [map][row][x], zero outside the volume
    __shared__ float XS[3 * HY * kLnTX];  // [map][row][x]

    const int chain = blockIdx.y;
    const int64_t V = (int64_t)g.D * g.H * g.W;
    const float* f = fixed + (int64_t)chain * fixed_stride;
    const float* m = moving + (int64_t)chain * V;
    const float* cc = coef + (int64_t)chain * 3 * V;
    float* go = g_moving + (int64_t)chain * V;
    const int tx = threadIdx.x & (kLnTX - 1), ty = threadIdx.x / kLnTX;

    for (int work = blockIdx.x; work < g.nwork; work += gridDim.x) {
        const int seg = work / g.tiles, tile = work - seg * g.tiles;
        const int x0 = (tile % g.tiles_x) * kLnTX, y0 = (tile / g.tiles_x) * kLnTY;
        const int z0 = seg * g.seg_len, z1 = min(z0 + g.seg_len, g.D);
        const int x = x0 + tx, y = y0 + ty;
        const bool inside = x < g.W && y < g.H;
        float ring[3][NT];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) ring[j][t] = 0.0f;
        for (int p = z0 - R; p < z1 + R; ++p) {
            float s[3] = {0.0f, 0.0f, 0.0f};
            if (p >= 0 && p < g.D) {  // (the same for every thread of the block)
                __syncthreads();      // T and XS of the plane before have been read
                for (int i = threadIdx.x; i < HX * HY; i += kBlock) {
                    const int hy = i / HX, hx = i - hy * HX;
                    const int gy = y0 + hy - R, gx = x0 + hx - R;
                    const bool in = gy >= 0 && gy < g.H && gx >= 0 && gx < g.W;
                    const int src = (p * g.H + gy) * g.W + gx;
#pragma unroll
                    for (int j = 0; j < 3; ++j) T[j * HY * HX + i] = in ? cc[j * V + src] : 0.0f;
                }
                __syncthreads();
                for (int i = threadIdx.x; i < kLnTX * HY; i += kBlock) {
                    const int hy = i / kLnTX, xx = i - hy * kLnTX;
                    float a[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const float w = fold_weight(x0 + xx, g.W, t - R, R);
#pragma unroll
                        for (int j = 0; j < 3; ++j) a[j] += w * T[j * HY * HX + hy * HX + xx + t];
                    }
#pragma unroll
                    for (int j = 0; j < 3; ++j) XS[j * HY * kLnTX + i] = a[j];
                }
                __syncthreads();
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float w = fold_weight(y, g.H, t - R, R);
#pragma unroll
                    for (int j = 0; j < 3; ++j) s[j] += w * XS[(j * HY + ty + t) * kLnTX + tx];
                }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
#pragma unroll
                for (int t = 0; t + 1 < NT; ++t) ring[j][t] = ring[j][t + 1];
                ring[j][NT - 1] = s[j];  // the newest plane last
            }
            const int z = p - R;
            if (z < z0 || !inside) continue;
            float b[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float w = fold_weight(z, g.D, t - R, R);
#pragma unroll
                for (int j = 0; j < 3; ++j) b[j] += w * ring[j][t];
            }
            const int v = (z * g.H + y) * g.W + x;
            go[v] = scale * ((m[v] * b[1] - f[v] * b[0]) - b[2]);
        }
    }
}

}  // namespace

LnccGeom lncc_geometry(int D, int H, int W, int radius) {
    LnccGeom g;
    g.D = D, g.H = H, g.W = W;
    g.tiles_x = (W + kLnTX - 1) / kLnTX;
    g.tiles = g.tiles_x * ((H + kLnTY - 1) / kLnTY);
    // z-segments: every segment re-stages 2 R planes, so none is shorter than 4 R; as many as fill the rows of partials.  The
    // `lcc_seg` switch forces a length (tests: a segment shorter than the window).
    const int forced = global_knobs().lcc_seg;
    if (forced > 0) {
        g.seg_len = std::min(forced, D);
    } else {
        const int want = (kMaxPartialBlocks + g.tiles - 1) / g.tiles;
        const int nseg = std::max(1, std::min(want, (D + 4 * radius - 1) / (4 * radius)));
        g.seg_len = (D + nseg - 1) / nseg;
    }
    g.nwork = g.tiles * ((D + g.seg_len - 1) / g.seg_len);
    g.blocks = std::min(g.nwork, kMaxPartialBlocks);
    return g;
}

void launch_lncc_fwd(const float* fixed, int64_t fixed_stride, const float* moving, const float* upstream, int64_t upstream_stride,
                     const uint8_t* mask, int64_t mask_stride, int radius, float eps, double scale, float* d, float* coef,
                     double* partials, int C, const LnccGeom& g, hipStream_t st) {
#define IRS_LNCC(RR)                                                                                                             \
    hipLaunchKernelGGL(lncc_fwd_kernel<RR>, dim3(g.blocks, C), dim3(kBlock), 0, st, fixed, fixed_stride, moving, upstream,      \
                       upstream_stride, mask, mask_stride, g, eps, scale, d, coef, partials)
    switch (radius) {
        case 1: IRS_LNCC(1); break;
        case 2: IRS_LNCC(2); break;
        case 3: IRS_LNCC(3); break;
        default: IRS_LNCC(4); break;
    }
#undef IRS_LNCC
}

void launch_lncc_bwd(const float* fixed, int64_t fixed_stride, const float* moving, const float* coef, int radius, float scale,
                     float* g_moving, int C, const LnccGeom& g, hipStream_t st) {
#define IRS_LNCC(RR) \
    hipLaunchKernelGGL(lncc_bwd_kernel<RR>, dim3(g.blocks, C), dim3(kBlock), 0, st, fixed, fixed_stride, moving, coef, g, scale, g_moving)
    switch (radius) {
        case 1: IRS_LNCC(1); break;
        case 2: IRS_LNCC(2); break;
        case 3: IRS_LNCC(3); break;
        default: IRS_LNCC(4); break;
    }
#undef IRS_LNCC
}

}  // namespace irs
