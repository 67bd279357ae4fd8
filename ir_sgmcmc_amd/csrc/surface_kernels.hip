// Surface posterior (absent in the reference): at every voxel of the fixed contour of a listed label, the Welford moments over
// the recorded chains of the signed distance to the moving contour of the same label.
//
//  - update: runs after the passes of metric_kernels.hip with KEEP, which leave the exact squared distance to the moving
//    contour B of every (chain, label) pair at every voxel of the pair's box (gB).  A gather: one thread per volume voxel on the
//    64 x 4 grid of the pointwise kernels, x fastest.  A thread leaves at once unless its voxel is on the fixed contour of a
//    listed label; else it loads its count / mean / m2 once, folds every chain's sample in chain order and stores once.  The
//    box of a pair holds every fixed voxel of its label, so the sample of chain c sits at a box-local index of pair c * L + l.
//    Each thread owns its voxel: no atomics, two calls on the same inputs are bit-identical.
//  - finalize: a wavefront per row, lanes on consecutive x, writes the two maps; the summary is segmented by label.  Lane j of
//    a wavefront keeps the accumulator of label j (L <= 64 = the wavefront): for every label among the 64 voxels of a step the
//    members' columns are reduced by the shuffle butterfly and merged into that lane.  The four wavefronts of a block are merged
//    in order into one row of partials per (label, block); one block per label folds its rows in index order.  Every merge has
//    a fixed order and the grid depends on the volume only: two calls are bit-identical.  No float atomics.
#include "contour_device.h"
#include "kernels.h"
#include "summary_device.h"

namespace irs {
namespace {

constexpr float kInf = __builtin_huge_valf();

// the index of the label value v in the table, -1 when it is not listed
__device__ __forceinline__ int label_index(const SurfLabels& lab, int L, int v) {
    for (int j = 0; j < L; ++j)
        if (lab.v[j] == v) return j;
    return -1;
}

__global__ __launch_bounds__(kBlock) void surface_update_kernel(const int16_t* __restrict__ F, const int16_t* __restrict__ M,
                                                                SurfLabels lab, int L, const SurfPair* __restrict__ plan,
                                                                const float* __restrict__ gB, int C, float* __restrict__ mean,
                                                                float* __restrict__ m2, int32_t* __restrict__ count, Vol vol) {
    IRS_VOXEL(vol, plane_, x, y, z, p);
    (void)plane_;
    const int f = F[p];
    const int li = label_index(lab, L, f);
    if (li < 0 || !on_contour(F, z, y, x, f, vol)) return;
    const int k0 = count[p];
    int k = k0;
    float mu = mean[p], s2 = m2[p];
    for (int c = 0; c < C; ++c) {
        const SurfPair q = plan[c * L + li];
        const int zz = z - q.z0, yy = y - q.y0, xx = x - q.x0;
        // the box of the pair holds every fixed voxel of its label; a table that does not fit the maps gives no sample
        if ((unsigned)zz >= (unsigned)q.nz || (unsigned)yy >= (unsigned)q.ny || (unsigned)xx >= (unsigned)q.nx) continue;
        const float d2 = gB[q.vox + ((int64_t)zz * q.ny + yy) * q.nx + xx];
        if (!(d2 < kInf)) continue;  // the label is absent from this chain's map
        const float d = (float)sqrt((double)d2);
        // negative where the fixed surface lies inside the warped structure; 0 on the moving contour itself
        const float s = d2 == 0.0f ? 0.0f : (M[(int64_t)c * vol.V + p] == f ? -d : d);
        ++k;
        const float delta = __fsub_rn(s, mu);
        mu = __fadd_rn(mu, __fdiv_rn(delta, (float)k));
        s2 = __fadd_rn(s2, __fmul_rn(delta, __fsub_rn(s, mu)));
    }
    if (k != k0) {
        count[p] = k;
        mean[p] = mu;
        m2[p] = s2;
    }
}

// the summary columns of one label: integer sums {contour voxels, voxels with count >= 1, voxels with count >= 2, voxels inside
// the band of each level}; then doubles {sum bias, sum |bias|, sum bias^2, max |bias|, sum std, max std}.  fmax never sees a
// NaN: a voxel enters a float column only where its value is defined.
struct SurfaceSummary {
    static constexpr int kInts = IRS_SURFACE_SUMMARY_INTS, kFloats = IRS_SURFACE_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 3 || j == 5 ? Col::Max : Col::Sum; }
};
using SurfAcc = SummaryAcc<SurfaceSummary>;
static_assert(IRS_SURFACE_SUMMARY_INTS == 3 + IRS_SURFACE_MAX_LEVELS, "one integer column per coverage level after the three counts");

// the butterfly of SummaryAcc::block_reduce over one wavefront, then lane 0's result in every lane
__device__ __forceinline__ SurfAcc wave_all_reduce(SurfAcc a) {
#pragma unroll
    for (int j = 0; j < SurfaceSummary::kInts; ++j) a.i[j] = __shfl(wave_sum_ll(a.i[j]), 0, kWave);
#pragma unroll
    for (int j = 0; j < SurfaceSummary::kFloats; ++j)
        a.f[j] = __shfl(SurfaceSummary::kind(j) == Col::Sum ? wave_sum(a.f[j]) : wave_max(a.f[j]), 0, kWave);
    return a;
}

__global__ __launch_bounds__(kBlock) void surface_finalize_kernel(const int16_t* __restrict__ F, SurfLabels lab, int L,
                                                                  const float* __restrict__ mean, const float* __restrict__ m2,
                                                                  const int32_t* __restrict__ count,
                                                                  const uint8_t* __restrict__ mask, SurfLevels lv,
                                                                  float* __restrict__ bias, float* __restrict__ std,
                                                                  long long* __restrict__ ipart, double* __restrict__ fpart,
                                                                  Vol vol) {
    __shared__ SurfAcc smem[kBlock];
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const float nan = __builtin_nanf("");
    SurfAcc mine = SurfAcc::identity();  // lane j: label j
    const int rows = vol.D * vol.H;
    for (int row = blockIdx.x * (kBlock / kWave) + wid; row < rows; row += gridDim.x * (kBlock / kWave)) {
        const int z = row / vol.H, y = row - z * vol.H;
        for (int cx = 0; cx < vol.W; cx += kWave) {  // whole wavefronts: the ballots below are uniform
            const int x = cx + lane;
            int li = -1;
            SurfAcc v = SurfAcc::identity();
            if (x < vol.W) {
                const int64_t p = (int64_t)row * vol.W + x;
                const int n = count[p];
                const float b = n >= 1 ? mean[p] : nan;
                const float sd = n >= 2 ? sqrtf(fmaxf(m2[p], 0.0f) / (float)(n - 1)) : nan;
                bias[p] = b;
                std[p] = sd;
                const int f = F[p];
                const int j = label_index(lab, L, f);
                if (j >= 0 && (!mask || mask[p]) && on_contour(F, z, y, x, f, vol)) {
                    li = j;
                    v.i[0] = 1;
                    if (n >= 1) {
                        const double bd = (double)b;
                        v.i[1] = 1;
                        v.f[0] = bd;
                        v.f[1] = fabs(bd);
                        v.f[2] = bd * bd;
                        v.f[3] = fabs(bd);
                    }
                    if (n >= 2) {
                        v.i[2] = 1;
                        v.f[4] = (double)sd;
                        v.f[5] = (double)sd;
#pragma unroll
                        for (int q = 0; q < IRS_SURFACE_MAX_LEVELS; ++q)
                            v.i[3 + q] = q < lv.n && fabs((double)b) <= lv.z[q] * (double)sd;
                    }
                }
            }
            uint64_t todo = __ballot(li >= 0);
            while (todo) {  // one turn per label among these 64 voxels, in the order of its first voxel
                const int j = __shfl(li, __builtin_ctzll(todo), kWave);
                const bool member = li == j;
                todo &= ~__ballot(member);
                const SurfAcc r = wave_all_reduce(member ? v : SurfAcc::identity());
                if (lane == j) mine.merge(r);
            }
        }
    }
    smem[threadIdx.x] = mine;
    __syncthreads();
    if (wid == 0 && lane < L) {
        for (int w = 1; w < kBlock / kWave; ++w) mine.merge(smem[w * kWave + lane]);
        mine.store(ipart, fpart, (int64_t)lane * gridDim.x + blockIdx.x);
    }
}

// one block per label: its rows of partials in index order
__global__ __launch_bounds__(kBlock) void surface_reduce_kernel(const long long* __restrict__ ipart, const double* __restrict__ fpart,
                                                                int nblocks, long long* __restrict__ isummary,
                                                                double* __restrict__ fsummary) {
    __shared__ SurfAcc smem[SurfAcc::kG];
    SurfAcc a = SurfAcc::identity();
    for (int b = threadIdx.x; b < nblocks; b += kBlock) a.merge(SurfAcc::load(ipart, fpart, (int64_t)blockIdx.x * nblocks + b));
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(isummary, fsummary, blockIdx.x);
}

}  // namespace

void launch_surface_posterior_update(const int16_t* fixed, const int16_t* moving, const SurfLabels& lab, int L, const SurfPair* plan,
                                     const float* gB, int C, float* mean, float* m2, int32_t* count, Vol vol, hipStream_t st) {
    hipLaunchKernelGGL(surface_update_kernel, vox_grid(vol, 1), dim3(kBlock), 0, st, fixed, moving, lab, L, plan, gB, C, mean, m2,
                       count, vol);
}

void launch_surface_posterior_finalize(const int16_t* fixed, const SurfLabels& lab, int L, const float* mean, const float* m2,
                                       const int32_t* count, const uint8_t* mask, const SurfLevels& lv, float* bias, float* std,
                                       long long* isummary, double* fsummary, void* ws, Vol vol, hipStream_t st) {
    const int64_t rows = (int64_t)vol.D * vol.H;
    const int blocks = (int)std::min<int64_t>((rows + kBlock / kWave - 1) / (kBlock / kWave), IRS_SURFACE_MAX_BLOCKS);
    long long* ipart = (long long*)ws;
    double* fpart = (double*)(ipart + (size_t)SurfaceSummary::kInts * blocks * L);
    hipLaunchKernelGGL(surface_finalize_kernel, dim3(blocks), dim3(kBlock), 0, st, fixed, lab, L, mean, m2, count, mask, lv, bias,
                       std, ipart, fpart, vol);
    hipLaunchKernelGGL(surface_reduce_kernel, dim3(L), dim3(kBlock), 0, st, ipart, fpart, blocks, isummary, fsummary);
}

}  // namespace irs
