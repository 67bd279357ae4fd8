// Local similarity maps of the fixed image and a (warped) moving image (absent in the reference, whose only windowed quantity
// is the LCC normalisation inside its data term): per chain and voxel the local normalised
// cross-correlation (LNCC) and SSIM over the (2R+1)^3 box window with clamped indices, their masked statistics, and the
// per-voxel posterior of the LNCC maps.
//
//  - map kernel: one launch for all chains, blockIdx.y the chain.  A work item is one 32 x 8 tile in x-y over one z-segment; a
//    block of 256 threads walks its work items (blockIdx.x, + gridDim.x, ...), one output column per thread, marching in z.
//    Per plane p of z0 - R .. z1 - 1 + R (clamped to the volume: the planes past an end are the end plane again):
//      A  the tile + halo R of both images, indices clamped in x and y, to LDS as float32 (TF, TM);
//      B  per element of the tile and its y-halo the five x-sums over 2R+1 neighbours -- f, m, f f, m m, f m, each float32
//         converted to double first, so every product is exact -- to LDS (XS);
//      C  per thread the five y-sums over 2R+1 rows of XS: the plane sums of its column, into slot p mod (2R+1) of the
//         thread's ring in LDS (5 (2R+1) doubles per thread do not fit the registers at R = 4);
//      D  the output plane z = p - R once it is inside the segment: the ring RE-SUMMED from the oldest plane to the newest --
//         no running z-sum, so a NaN or inf leaves with the plane that brought it -- then the means, variances, LNCC and SSIM
//         in double, rounded once on the store.
//    A window holding a non-finite value has a non-finite S_ff or S_mm (a finite float32 squared and summed 729 times cannot
//    overflow a double), which is how it is recognised.  The statistics stay in registers (SummaryAcc, summary_device.h): one
//    row of partials per block and chain.
//  - stats kernel: the second stage, one block per chain: thread i folds rows i, i + 256, ... in order, the block reduction of
//    summary_device.h, then the seven doubles of the chain.
//  - update / finalize: the streaming mean, minimum and count of the LNCC samples per voxel, and their masked summary.
// LDS per block, R = 1 / 2 / 3 / 4: 45 / 69 / 92 / 115 KB of the CU's 160 -- 3 / 2 / 1 / 1 blocks of four wavefronts per CU.
// Two identical calls are bit-identical and chain c of a batch equals the single-chain call: the grid and every order of
// summation depend on (D, H, W, R) only.
#include <algorithm>

#include "kernels.h"
#include "summary_device.h"

namespace irs {
namespace {

// integer sums {voxels of the mask with a finite window, flat ones among them, voxels of the mask with a non-finite window};
// doubles {sum LNCC, min LNCC} over the defined voxels and {sum SSIM, min SSIM} over the finite ones (fmin never sees a NaN)
struct LocalSummary {
    static constexpr int kInts = 3, kFloats = 4;
    static constexpr Col kind(int j) { return (j & 1) ? Col::Min : Col::Sum; }
};
using LocalAcc = SummaryAcc<LocalSummary>;
static_assert(LocalSummary::kInts + LocalSummary::kFloats == IRS_LOCAL_STATS, "one statistic per summary column");

// over the mask: integer sums {voxels, voxels with count == 0}; doubles over the others {sum mean, min mean, min low}
struct LocalMapSummary {
    static constexpr int kInts = IRS_LOCAL_MAP_SUMMARY_INTS, kFloats = IRS_LOCAL_MAP_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 0 ? Col::Sum : Col::Min; }
};
using LocalMapAcc = SummaryAcc<LocalMapSummary>;

constexpr int kLocTX = 32, kLocTY = 8;  // the tile: one output column per thread
static_assert(kLocTX * kLocTY == kBlock, "one thread per column of the tile");

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

template <int R>
__global__ __launch_bounds__(kBlock) void local_similarity_kernel(const float* __restrict__ fixed, int64_t fixed_stride,
                                                                  const float* __restrict__ moving,
                                                                  const uint8_t* __restrict__ mask, LocalGeom g, LocalConsts k,
                                                                  float* __restrict__ lncc, float* __restrict__ ssim,
                                                                  long long* __restrict__ ipart, double* __restrict__ fpart) {
    constexpr int NT = 2 * R + 1, HX = kLocTX + 2 * R, HY = kLocTY + 2 * R;
    __shared__ double ring[5 * NT * kBlock];    // [sum][slot][thread]
    __shared__ double XS[5 * HY * kLocTX];      // [sum][row][x]
    __shared__ float TF[HY * HX], TM[HY * HX];  // [row][x]
    __shared__ LocalAcc smem[LocalAcc::kG];

    const int chain = blockIdx.y;
    const int64_t V = (int64_t)g.D * g.H * g.W;
    const float* f = fixed + (int64_t)chain * fixed_stride;
    const float* m = moving + (int64_t)chain * V;
    float* lo = lncc ? lncc + (int64_t)chain * V : nullptr;
    float* so = ssim ? ssim + (int64_t)chain * V : nullptr;
    const int tx = threadIdx.x & (kLocTX - 1), ty = threadIdx.x / kLocTX;
    const double n = (double)(NT * NT * NT);
    const float nanf_ = __builtin_nanf("");
    LocalAcc a = LocalAcc::identity();

    for (int work = blockIdx.x; work < g.nwork; work += gridDim.x) {
        const int seg = work / g.tiles, tile = work - seg * g.tiles;
        const int x0 = (tile % g.tiles_x) * kLocTX, y0 = (tile / g.tiles_x) * kLocTY;
        const int z0 = seg * g.seg_len, z1 = min(z0 + g.seg_len, g.D);
        const int x = x0 + tx, y = y0 + ty;
        const bool inside = x < g.W && y < g.H;
        int slot = 0;
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
            for (int i = threadIdx.x; i < kLocTX * HY; i += kBlock) {
                const int hy = i / kLocTX, xx = i - hy * kLocTX;
                double sf = 0.0, sm = 0.0, sff = 0.0, smm = 0.0, sfm = 0.0;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const double vf = (double)TF[hy * HX + xx + t], vm = (double)TM[hy * HX + xx + t];
                    sf += vf;
                    sm += vm;
                    sff += vf * vf;
                    smm += vm * vm;
                    sfm += vf * vm;
                }
                XS[0 * HY * kLocTX + i] = sf;
                XS[1 * HY * kLocTX + i] = sm;
                XS[2 * HY * kLocTX + i] = sff;
                XS[3 * HY * kLocTX + i] = smm;
                XS[4 * HY * kLocTX + i] = sfm;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                double s = 0.0;
#pragma unroll
                for (int t = 0; t < NT; ++t) s += XS[(q * HY + ty + t) * kLocTX + tx];
                ring[(q * NT + slot) * kBlock + threadIdx.x] = s;  // the thread's own: no barrier
            }
            slot = slot + 1 == NT ? 0 : slot + 1;  // now the oldest plane of the ring
            const int z = p - R;
            if (z < z0) continue;
            double S[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                double s = 0.0;
                int sl = slot;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    s += ring[(q * NT + sl) * kBlock + threadIdx.x];
                    sl = sl + 1 == NT ? 0 : sl + 1;
                }
                S[q] = s;
            }
            if (!inside) continue;
            const bool finite = isfinite(S[2]) && isfinite(S[3]);
            const double mf = S[0] / n, mm = S[1] / n;
            const double var_f = fmax(S[2] / n - mf * mf, 0.0), var_m = fmax(S[3] / n - mm * mm, 0.0);
            const double cov = S[4] / n - mf * mm;
            const bool flat = !(var_f > k.floor_f && var_m > k.floor_m);
            const double lv = fmin(fmax(cov / sqrt(var_f * var_m), -1.0), 1.0);
            const double sv = ((2.0 * mf * mm + k.c1) * (2.0 * cov + k.c2)) / ((mf * mf + mm * mm + k.c1) * (var_f + var_m + k.c2));
            const int v = (z * g.H + y) * g.W + x;
            if (lo) lo[v] = finite && !flat ? (float)lv : nanf_;
            if (so) so[v] = finite ? (float)sv : nanf_;
            if (!mask || mask[v]) {
                if (finite) {
                    a.i[0] += 1;
                    if (flat) {
                        a.i[1] += 1;
                    } else {
                        a.f[0] += lv;
                        a.f[1] = fmin(a.f[1], lv);
                    }
                    a.f[2] += sv;
                    a.f[3] = fmin(a.f[3], sv);
                } else {
                    a.i[2] += 1;
                }
            }
        }
    }
    __syncthreads();
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, (int64_t)chain * gridDim.x + blockIdx.x);
}

// the chain's `nblocks` rows of partials -> its IRS_LOCAL_STATS doubles.  One block per chain.
__global__ __launch_bounds__(kBlock) void local_similarity_stats_kernel(const long long* __restrict__ ipart,
                                                                        const double* __restrict__ fpart, int nblocks,
                                                                        double* __restrict__ stats) {
    __shared__ LocalAcc smem[LocalAcc::kG];
    const int chain = blockIdx.x;
    LocalAcc a = LocalAcc::identity();
    for (int b = threadIdx.x; b < nblocks; b += kBlock) a.merge(LocalAcc::load(ipart, fpart, (int64_t)chain * nblocks + b));
    a.block_reduce(smem);
    if (threadIdx.x == 0) {
        double* s = stats + (int64_t)chain * IRS_LOCAL_STATS;
        const double nan = __builtin_nan("");
        const long long defined = a.i[0] - a.i[1];
        s[0] = (double)a.i[0];
        s[1] = (double)a.i[1];
        s[2] = (double)a.i[2];
        s[3] = defined > 0 ? a.f[0] / (double)defined : nan;
        s[4] = a.f[1];
        s[5] = a.i[0] > 0 ? a.f[2] / (double)a.i[0] : nan;
        s[6] = a.f[3];
    }
}

// lncc (C,V) -> mean, low (V) float32 and count (V) int32: each thread owns its voxels, the chains folded in order, a NaN
// sample skipped
__global__ __launch_bounds__(kBlock) void local_similarity_update_kernel(const float* __restrict__ lncc, int C, int64_t V,
                                                                         float* __restrict__ mean, float* __restrict__ low,
                                                                         int32_t* __restrict__ count, int records_before) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        float mu = 0.0f, lw = INFINITY;
        int n = 0;
        if (records_before > 0) {
            mu = mean[v];
            lw = low[v];
            n = count[v];
        }
        for (int c = 0; c < C; ++c) {
            const float x = lncc[(int64_t)c * V + v];
            if (isnan(x)) continue;
            ++n;
            mu = __fadd_rn(mu, __fsub_rn(x, mu) / (float)n);
            lw = fminf(lw, x);
        }
        mean[v] = mu;
        low[v] = lw;
        count[v] = n;
    }
}

__global__ __launch_bounds__(kBlock) void local_similarity_finalize_kernel(const float* __restrict__ mean,
                                                                           const float* __restrict__ low,
                                                                           const int32_t* __restrict__ count, int64_t V,
                                                                           const uint8_t* __restrict__ mask,
                                                                           long long* __restrict__ ipart,
                                                                           double* __restrict__ fpart) {
    __shared__ LocalMapAcc smem[LocalMapAcc::kG];
    LocalMapAcc a = LocalMapAcc::identity();
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[v]) continue;
        a.i[0] += 1;
        if (count[v] > 0) {  // every sample folded in was no NaN: neither is the mean or the minimum
            const double mu = (double)mean[v];
            a.f[0] += mu;
            a.f[1] = fmin(a.f[1], mu);
            a.f[2] = fmin(a.f[2], (double)low[v]);
        } else {
            a.i[1] += 1;
        }
    }
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, blockIdx.x);
}

}  // namespace

LocalGeom local_similarity_geometry(int D, int H, int W, int radius) {
    LocalGeom g;
    g.D = D, g.H = H, g.W = W;
    g.tiles_x = (W + kLocTX - 1) / kLocTX;
    g.tiles = g.tiles_x * ((H + kLocTY - 1) / kLocTY);
    // z-segments: every segment re-stages 2 R planes, so none is shorter than 8 R; as many as fill the rows of partials
    const int want = (IRS_LOCAL_MAX_BLOCKS + g.tiles - 1) / g.tiles;
    const int nseg = std::max(1, std::min(want, (D + 8 * radius - 1) / (8 * radius)));
    g.seg_len = (D + nseg - 1) / nseg;
    g.nwork = g.tiles * ((D + g.seg_len - 1) / g.seg_len);
    g.blocks = std::min(g.nwork, IRS_LOCAL_MAX_BLOCKS);
    return g;
}

void launch_local_similarity(const float* fixed, int64_t fixed_stride, const float* moving, const uint8_t* mask, int C, int radius,
                             const LocalGeom& g, const LocalConsts& k, float* lncc, float* ssim, double* stats, void* ws,
                             hipStream_t st) {
    long long* ipart = (long long*)ws;
    double* fpart = (double*)(ipart + (size_t)LocalSummary::kInts * g.blocks * C);
#define IRS_LOCAL(RR)                                                                                                          \
    hipLaunchKernelGGL(local_similarity_kernel<RR>, dim3(g.blocks, C), dim3(kBlock), 0, st, fixed, fixed_stride, moving, mask, \
                       g, k, lncc, ssim, ipart, fpart)
    switch (radius) {
        case 1: IRS_LOCAL(1); break;
        case 2: IRS_LOCAL(2); break;
        case 3: IRS_LOCAL(3); break;
        default: IRS_LOCAL(4); break;
    }
#undef IRS_LOCAL
    hipLaunchKernelGGL(local_similarity_stats_kernel, dim3(C), dim3(kBlock), 0, st, ipart, fpart, g.blocks, stats);
}

static int local_stream_blocks(int64_t n) { return (int)std::min<int64_t>((n + kBlock - 1) / kBlock, 4096); }

void launch_local_similarity_update(const float* lncc, int C, int64_t V, float* mean, float* low, int32_t* count,
                                    int records_before, hipStream_t st) {
    hipLaunchKernelGGL(local_similarity_update_kernel, dim3(local_stream_blocks(V)), dim3(kBlock), 0, st, lncc, C, V, mean, low,
                       count, records_before);
}

void launch_local_similarity_finalize(const float* mean, const float* low, const int32_t* count, int64_t V, const uint8_t* mask,
                                      long long* isummary, double* fsummary, void* ws, hipStream_t st) {
    const SummaryPartials<LocalMapSummary> part(V, ws, IRS_LOCAL_MAP_WS_BYTES);
    hipLaunchKernelGGL(local_similarity_finalize_kernel, dim3(part.blocks), dim3(kBlock), 0, st, mean, low, count, V, mask,
                       part.ipart, part.fpart);
    part.reduce(isummary, fsummary, st);
}

}  // namespace irs
