// Structure report (absent in the reference): per structure of the fixed segmentation, the sums behind the posterior of its mean
// displacement and of its volume change, one labelled reduction per recorded sample, and the same reduction over finished
// per-voxel maps ("Structure report").
//
//  - motion: grid (blocks, C).  A grid-stride stream over the voxels of one chain, one voxel per thread and round: the three
//    displacement channels, the 3 x 3 forward-difference stencil of the transformation (jacobian_device.h), the label and the
//    mask; then the labelled reduction of structure_device.h.
//  - map statistics: grid (blocks, M), the same stream over one map.
//  - both end in structure_fold_kernel, one block per (structure, row), over the blocks' partials.
// The grid depends on the volume alone (min(ceil(V / 256), 1024) blocks per row), every merge has a fixed place: two identical
// calls are bit-identical.  A grid's second dimension holds 65535 rows; more rows are launched in turns.
#include <algorithm>

#include "structure_device.h"

namespace irs {
namespace {

constexpr int kMaxGridRows = 65535;

// u, t (C,3,V) float32; seg (V) int16; mask (V) uint8 or nullptr; partials: structure_device.h
__global__ __launch_bounds__(kBlock) void structure_motion_kernel(const float* __restrict__ u, const float* __restrict__ t,
                                                                  const int16_t* __restrict__ seg, const uint8_t* __restrict__ mask,
                                                                  SurfLabels lab, int K, double s0, double s1, double s2, Vol vol,
                                                                  int64_t row0, long long* __restrict__ ipart,
                                                                  double* __restrict__ fpart) {
    __shared__ StructureTables<StructureMotion> tab;
    tab.clear(K);
    const int64_t row = row0 + blockIdx.y;
    const float* uc = u + row * 3 * vol.V;
    const float* tc = t + row * 3 * vol.V;
    const double scale[3] = {s0, s1, s2};
    const int V = (int)vol.V;  // < 2^30 (api_checks.h: dims_ok)
    // `base` is uniform over the block: every lane of a wavefront reaches the fold of every round
    for (int base = blockIdx.x * kBlock; base < V; base += gridDim.x * kBlock) {
        const int p = base + threadIdx.x;
        int j = -1;
        SummaryAcc<StructureMotion> a = SummaryAcc<StructureMotion>::identity();
        if (p < V) {
            j = structure_at(seg, mask, p, lab, K);
            if (j >= 0) {
                const int q = p / vol.W, x = p - q * vol.W, z = q / vol.H, y = q - z * vol.H;
                a = structure_motion_voxel(uc, tc, p, x, y, z, scale, vol);
            }
        }
        structure_wave_fold(j, a, tab);
    }
    structure_block_store(tab, K, row, ipart, fpart);
}

// maps (M,V) float32
__global__ __launch_bounds__(kBlock) void structure_map_stats_kernel(const float* __restrict__ maps, const int16_t* __restrict__ seg,
                                                                     const uint8_t* __restrict__ mask, SurfLabels lab, int K, int64_t V,
                                                                     int64_t row0, long long* __restrict__ ipart,
                                                                     double* __restrict__ fpart) {
    __shared__ StructureTables<StructureMapStats> tab;
    tab.clear(K);
    const int64_t row = row0 + blockIdx.y;
    const float* m = maps + row * V;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < V; base += (int64_t)gridDim.x * kBlock) {
        const int64_t p = base + threadIdx.x;
        int j = -1;
        SummaryAcc<StructureMapStats> a = SummaryAcc<StructureMapStats>::identity();
        if (p < V) {
            j = structure_at(seg, mask, p, lab, K);
            if (j >= 0) a = structure_map_voxel(m[p]);
        }
        structure_wave_fold(j, a, tab);
    }
    structure_block_store(tab, K, row, ipart, fpart);
}

template <class T>
struct Partials {
    int blocks;
    long long* ipart;
    double* fpart;
    Partials(int64_t V, int K, int64_t rows, void* ws)
        : blocks(structure_blocks(V)), ipart((long long*)ws), fpart((double*)(ipart + (size_t)rows * K * blocks * T::kInts)) {}
};

}  // namespace

int structure_blocks(int64_t V) { return (int)std::min<int64_t>((V + kBlock - 1) / kBlock, kStructureMaxBlocks); }

size_t structure_workspace_bytes(int64_t V, int K, int64_t rows) {
    constexpr int cols = std::max(IRS_STRUCTURE_MOTION_INTS + IRS_STRUCTURE_MOTION_FLOATS, IRS_STRUCTURE_MAP_INTS + IRS_STRUCTURE_MAP_FLOATS);
    return sizeof(double) * cols * (size_t)rows * K * structure_blocks(V);
}

void launch_structure_motion(const float* displacement, const float* transformation, const int16_t* seg_fixed, const SurfLabels& lab,
                             int K, const uint8_t* mask, const float* scale, long long* ints, double* floats, void* ws, int C, Vol vol,
                             hipStream_t st) {
    const Partials<StructureMotion> part(vol.V, K, C, ws);
    hipLaunchKernelGGL(structure_motion_kernel, dim3(part.blocks, C), dim3(kBlock), 0, st, displacement, transformation, seg_fixed, mask,
                       lab, K, (double)scale[0], (double)scale[1], (double)scale[2], vol, (int64_t)0, part.ipart, part.fpart);
    hipLaunchKernelGGL(structure_fold_kernel<StructureMotion>, dim3(K, C), dim3(kBlock), 0, st, part.ipart, part.fpart, part.blocks, K,
                       (int64_t)0, ints, floats);
}

void launch_structure_map_stats(const float* maps, int64_t M, int64_t V, const int16_t* seg_fixed, const SurfLabels& lab, int K,
                                const uint8_t* mask, long long* ints, double* floats, void* ws, hipStream_t st) {
    const Partials<StructureMapStats> part(V, K, M, ws);
    for (int64_t row0 = 0; row0 < M; row0 += kMaxGridRows) {
        const unsigned rows = (unsigned)std::min<int64_t>(M - row0, kMaxGridRows);
        hipLaunchKernelGGL(structure_map_stats_kernel, dim3(part.blocks, rows), dim3(kBlock), 0, st, maps, seg_fixed, mask, lab, K, V,
                           row0, part.ipart, part.fpart);
        hipLaunchKernelGGL(structure_fold_kernel<StructureMapStats>, dim3(K, rows), dim3(kBlock), 0, st, part.ipart, part.fpart,
                           part.blocks, K, row0, ints, floats);
    }
}

}  // namespace irs
