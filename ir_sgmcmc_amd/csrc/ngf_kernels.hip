// The NGF data term (absent in the reference): the normalised gradient field distance of Haber & Modersitzki
// (2006) and its exact adjoint with respect to the moving image.  It compares only the DIRECTION of the two image gradients, up to
// their sign: local like LNCC, contrast-free like MI.  All of it float32, as include/irsgmcmc.h states it and ngf_device.h spells it
// out operation by operation:
//   a = grad F, b = grad M (clamped central differences), P = a.b, Nf = |a|^2 + eps_f^2, Nm = |b|^2 + eps_m^2
//   r = P / (Nf Nm), d = 1 - P r, s = P / Nm, k = -2 u r, c = k (a - s b), g_M = grad^T c
// Both kernels are z-marching column tiles with the launch shape of lncc_kernels.hip (lncc_geometry at radius 1): a work item is one
// 32 x 8 tile in x-y over one z-segment, a block of 256 threads walks its work items (blockIdx.x, + gridDim.x, ...), one column per
// thread; blockIdx.y is the chain, so every chain runs in the one launch.
//  - forward kernel, per plane p of z0 - 1 .. z1 (clamped: a plane past an end is the end plane again): tile + halo 1 of F and M,
//    indices clamped in x and y, to LDS; every thread reads its own voxel and the y and x differences of that plane from LDS.  The
//    own voxel goes into a ring of three planes in registers (shifted by one per plane, every index static: no scratch), the
//    in-plane differences wait one plane; the output plane z = p - 1 takes its z difference from the ring's ends.  It writes c,
//    optionally d, and u d into the thread's double: one double of sum u d per workgroup and chain, summed in a fixed order
//    (block_sum), then scaled.
//  - adjoint kernel: needs neither image.  c_z of the own column through a ring of three planes in registers, read straight from
//    global memory; c_y of the plane with a one-row halo and c_x with a one-column halo, indices clamped, through LDS.  The face
//    rules are the tap weights -1 / +1 of ngf_device.h on the clamped neighbours, no branch.
// Global accesses are 4-byte loads and stores, 32 consecutive floats per row of a tile, with one exception.  The halo column shifts
// the staged rows of F, M and c_x by one float off every 16-byte boundary, and the c_z ring is one voxel per lane by the
// one-column-per-thread shape; the adjoint's c_y tile (row base x0, a multiple of 32) is the one array a 16-byte load fits: for
// W % 4 == 0 and a full tile 80 lanes stage it with one 16-byte load each (measured: 61.9 against 69.8 us at 256^3).
// No atomics and no state: the grid and every order of summation depend on (D, H, W) and the segment length only, so two identical
// calls are bit-identical and chain c of a batch equals the single-chain call.
#include <algorithm>
#include <cstdint>

#include "kernels.h"
#include "ngf_device.h"

namespace irs {
namespace {

constexpr int kNgTX = 32, kNgTY = 8;  // the tile: one column per thread
static_assert(kNgTX * kNgTY == kBlock, "one thread per column of the tile");

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

__global__ __launch_bounds__(kBlock) void ngf_fwd_kernel(const float* __restrict__ fixed, int64_t fixed_stride,
                                                         const float* __restrict__ moving, const float* __restrict__ upstream,
                                                         int64_t upstream_stride, const uint8_t* __restrict__ mask,
                                                         int64_t mask_stride, LnccGeom g, float ef2, float em2, double scale,
                                                         int weighted_map, float* __restrict__ d_out, float* __restrict__ coef,
                                                         double* __restrict__ partials) {
    constexpr int HX = kNgTX + 2, HY = kNgTY + 2;
    __shared__ float TF[HY * HX], TM[HY * HX];  // [row][x]
    __shared__ double smem[kBlock / kWave];

    const int chain = blockIdx.y;
    const int64_t V = (int64_t)g.D * g.H * g.W;
    const float* f = fixed + (int64_t)chain * fixed_stride;
    const float* m = moving + (int64_t)chain * V;
    const float* up = upstream ? upstream + (int64_t)chain * upstream_stride : nullptr;
    const uint8_t* mk = mask ? mask + (int64_t)chain * mask_stride : nullptr;
    float* dc = d_out ? d_out + (int64_t)chain * V : nullptr;
    float* cc = coef ? coef + (int64_t)chain * 3 * V : nullptr;
    const int tx = threadIdx.x & (kNgTX - 1), ty = threadIdx.x / kNgTX;
    const int li = (ty + 1) * HX + tx + 1;  // the thread's own voxel in the staged tile
    double acc[1] = {0.0};

    for (int work = blockIdx.x; work < g.nwork; work += gridDim.x) {
        const int seg = work / g.tiles, tile = work - seg * g.tiles;
        const int x0 = (tile % g.tiles_x) * kNgTX, y0 = (tile / g.tiles_x) * kNgTY;
        const int z0 = seg * g.seg_len, z1 = min(z0 + g.seg_len, g.D);
        const int x = x0 + tx, y = y0 + ty;
        const bool inside = x < g.W && y < g.H;
        float f0 = 0.0f, f1 = 0.0f, m0 = 0.0f, m1 = 0.0f;          // the ring: planes p - 2 and p - 1 of the own column
        float fy1 = 0.0f, fx1 = 0.0f, my1 = 0.0f, mx1 = 0.0f;      // the in-plane differences of plane p - 1
        for (int p = z0 - 1; p <= z1; ++p) {
            const int plane = clampi(p, g.D - 1) * g.H;
            __syncthreads();  // the tiles of the plane before have been read
            for (int i = threadIdx.x; i < HX * HY; i += kBlock) {
                const int hy = i / HX, hx = i - hy * HX;
                const int src = (plane + clampi(y0 + hy - 1, g.H - 1)) * g.W + clampi(x0 + hx - 1, g.W - 1);
                TF[i] = f[src];
                TM[i] = m[src];
            }
            __syncthreads();
            const float f2 = TF[li], m2 = TM[li];
            const float fy2 = ngf_diff(TF[li + HX], TF[li - HX]), fx2 = ngf_diff(TF[li + 1], TF[li - 1]);
            const float my2 = ngf_diff(TM[li + HX], TM[li - HX]), mx2 = ngf_diff(TM[li + 1], TM[li - 1]);
            const int z = p - 1;
            if (z >= z0 && inside) {
                const int v = (z * g.H + y) * g.W + x;
                const float u = up ? up[v] : mk ? (float)mk[v] : 1.0f;
                const float a[3] = {ngf_diff(f2, f0), fy1, fx1}, b[3] = {ngf_diff(m2, m0), my1, mx1};
                float d, c[3];
                ngf_point(a, b, u, ef2, em2, d, c);
                if (cc) {
                    cc[v] = c[0];
                    cc[V + v] = c[1];
                    cc[2 * V + v] = c[2];
                }
                if (dc) dc[v] = weighted_map ? __fmul_rn(u, d) : d;
                acc[0] += (double)u * (double)d;
            }
            f0 = f1, f1 = f2, m0 = m1, m1 = m2;
            fy1 = fy2, fx1 = fx2, my1 = my2, mx1 = mx2;
        }
    }
    if (!partials) return;
    __syncthreads();
    block_sum<1>(acc, smem);
    if (threadIdx.x == 0) partials[(int64_t)chain * gridDim.x + blockIdx.x] = scale * acc[0];
}

__global__ __launch_bounds__(kBlock) void ngf_bwd_kernel(const float* __restrict__ coef, LnccGeom g, float scale,
                                                         float* __restrict__ g_moving, int vec) {
    constexpr int HX = kNgTX + 2, HY = kNgTY + 2;
    __shared__ __align__(16) float TY[HY * kNgTX];  // c_y: [row - 1][x]
    __shared__ float TX[kNgTY * HX];  // c_x: [row][x - 1]

    const int chain = blockIdx.y;
    const int64_t V = (int64_t)g.D * g.H * g.W;
    const float* cz = coef + (int64_t)chain * 3 * V;
    const float* cy = cz + V;
    const float* cx = cz + 2 * V;
    float* go = g_moving + (int64_t)chain * V;
    const int tx = threadIdx.x & (kNgTX - 1), ty = threadIdx.x / kNgTX;

    for (int work = blockIdx.x; work < g.nwork; work += gridDim.x) {
        const int seg = work / g.tiles, tile = work - seg * g.tiles;
        const int x0 = (tile % g.tiles_x) * kNgTX, y0 = (tile / g.tiles_x) * kNgTY;
        const int z0 = seg * g.seg_len, z1 = min(z0 + g.seg_len, g.D);
        const int x = x0 + tx, y = y0 + ty;
        const bool inside = x < g.W && y < g.H;
        const int col = min(y, g.H - 1) * g.W + min(x, g.W - 1);  // (a thread outside the volume reads a voxel that exists)
        const float sxm = ngf_tap_lo(x), sxp = ngf_tap_hi(x, g.W), sym = ngf_tap_lo(y), syp = ngf_tap_hi(y, g.H);
        float r0 = cz[clampi(z0 - 1, g.D - 1) * g.H * g.W + col], r1 = cz[z0 * g.H * g.W + col];  // the ring: planes z - 1 and z
        for (int z = z0; z < z1; ++z) {
            const float r2 = cz[clampi(z + 1, g.D - 1) * g.H * g.W + col];
            const int plane = z * g.H;
            __syncthreads();  // the tiles of the plane before have been read
            if (vec && x0 + kNgTX <= g.W) {  // a full tile, rows 16-byte aligned: one 16-byte load per four floats, 80 lanes per plane
                if (threadIdx.x < HY * (kNgTX / 4)) {
                    const int hy = threadIdx.x / (kNgTX / 4), k = threadIdx.x - hy * (kNgTX / 4);
                    const float4 q = *reinterpret_cast<const float4*>(cy + (plane + clampi(y0 + hy - 1, g.H - 1)) * g.W + x0 + 4 * k);
                    *reinterpret_cast<float4*>(TY + hy * kNgTX + 4 * k) = q;
                }
            } else
                for (int i = threadIdx.x; i < HY * kNgTX; i += kBlock) {
                    const int hy = i / kNgTX, xx = i - hy * kNgTX;
                    TY[i] = cy[(plane + clampi(y0 + hy - 1, g.H - 1)) * g.W + min(x0 + xx, g.W - 1)];
                }
            for (int i = threadIdx.x; i < kNgTY * HX; i += kBlock) {
                const int hy = i / HX, hx = i - hy * HX;
                TX[i] = cx[(plane + min(y0 + hy, g.H - 1)) * g.W + clampi(x0 + hx - 1, g.W - 1)];
            }
            __syncthreads();
            if (inside) {
                const float gz = ngf_adjoint_axis(r0, r2, ngf_tap_lo(z), ngf_tap_hi(z, g.D));
                const float gy = ngf_adjoint_axis(TY[ty * kNgTX + tx], TY[(ty + 2) * kNgTX + tx], sym, syp);
                const float gx = ngf_adjoint_axis(TX[ty * HX + tx], TX[ty * HX + tx + 2], sxm, sxp);
                go[(plane + y) * g.W + x] = __fmul_rn(scale, __fadd_rn(__fadd_rn(gz, gy), gx));
            }
            r0 = r1, r1 = r2;
        }
    }
}

}  // namespace

void launch_ngf_fwd(const float* fixed, int64_t fixed_stride, const float* moving, const float* upstream, int64_t upstream_stride,
                    const uint8_t* mask, int64_t mask_stride, float eps_f, float eps_m, double scale, bool weighted_map, float* d,
                    float* coef, double* partials, int C, const LnccGeom& g, hipStream_t st) {
    const float ef2 = eps_f * eps_f, em2 = eps_m * eps_m;  // (float32 products, each rounded once, as the restatement forms them)
    hipLaunchKernelGGL(ngf_fwd_kernel, dim3(g.blocks, C), dim3(kBlock), 0, st, fixed, fixed_stride, moving, upstream, upstream_stride,
                       mask, mask_stride, g, ef2, em2, scale, weighted_map ? 1 : 0, d, coef, partials);
}

void launch_ngf_bwd(const float* coef, float scale, float* g_moving, int C, const LnccGeom& g, hipStream_t st) {
    // 16-byte loads of the c_y tile where every row of it starts on a 16-byte boundary: W a multiple of 4 (then V is one too, and so
    // is the offset of c_y in a chain's maps) and the maps themselves aligned
    const int vec = g.W % 4 == 0 && ((uintptr_t)coef & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(ngf_bwd_kernel, dim3(g.blocks, C), dim3(kBlock), 0, st, coef, g, scale, g_moving, vec);
}

}  // namespace irs
