// Device arithmetic of the structure report (structure_kernels.hip): the per-voxel columns of the two reductions and the
// labelled reduction they share.
//
// A family describes its columns as summary_device.h does (T::kInts int64 sums, T::kFloats doubles, each a sum, a maximum or
// a minimum by T::kind).  The first stage is a grid-stride stream over the voxels of one row (a chain, or a map): a thread forms
// the SummaryAcc<T> of its voxel and the structure j it belongs to (-1: none), and structure_wave_fold reduces, per wavefront
// and per distinct structure present in it, the members' columns by the shuffle butterfly -- non-members contribute the
// identity -- and lane 0 merges the result into the wavefront's OWN table in LDS.  structure_block_store merges the four
// tables in wavefront order and writes the block's row of partials; structure_fold_kernel folds the rows of one (row,
// structure) in block order exactly as summary_reduce_kernel does.  No floating-point atomics anywhere: every addition has a
// fixed place in a fixed order, so two identical calls are bit-identical, and the integer columns are exact.
#pragma once
#include "jacobian_device.h"
#include "label_device.h"
#include "summary_device.h"

namespace irs {

constexpr int kStructureMaxBlocks = 1024;  // 256 CUs x 4 blocks of 4 wavefronts; rows of partials per (row, structure)
constexpr int kStructureWaves = kBlock / kWave;

// {voxels, folded}; {sum w_x, sum w_y, sum w_z, sum |w|, sum |w|^2, max |w|, sum det, min det, max det}
struct StructureMotion {
    static constexpr int kInts = IRS_STRUCTURE_MOTION_INTS, kFloats = IRS_STRUCTURE_MOTION_FLOATS;
    static constexpr Col kind(int j) { return j == 5 || j == 8 ? Col::Max : j == 7 ? Col::Min : Col::Sum; }
};
// {finite, non_finite}; {sum x, sum x^2, min, max} over the finite values
struct StructureMapStats {
    static constexpr int kInts = IRS_STRUCTURE_MAP_INTS, kFloats = IRS_STRUCTURE_MAP_FLOATS;
    static constexpr Col kind(int j) { return j == 2 ? Col::Min : j == 3 ? Col::Max : Col::Sum; }
};

// the structure of voxel p: seg[p] == labels[j] and, with a mask, mask[p] != 0; every other voxel belongs to none (-1)
__device__ __forceinline__ int structure_at(const int16_t* __restrict__ seg, const uint8_t* __restrict__ mask, int64_t p,
                                            const SurfLabels& lab, int K) {
    if (mask && !mask[p]) return -1;
    return structure_of(seg[p], lab, K);
}

// one voxel of one chain.  w_c = (double)u_c * (double)scale_c is exact (24 x 24 bits); |w|^2 = (w_x^2 + w_y^2) + w_z^2 and
// |w| = sqrt(|w|^2) in double, every operation rounded on its own (no contraction: the host restatement is the same bits).
// det: det_jacobian in float32, converted.  Folded when !(det > 0), NaN included; a NaN det stays out of the det columns.
// A non-finite displacement propagates into the sums (the maximum drops a NaN, as fmax does).
__device__ __forceinline__ SummaryAcc<StructureMotion> structure_motion_voxel(const float* __restrict__ u, const float* __restrict__ t,
                                                                              int64_t p, int x, int y, int z, const double (&scale)[3],
                                                                              const Vol& vol) {
    SummaryAcc<StructureMotion> a = SummaryAcc<StructureMotion>::identity();
    const double wx = __dmul_rn((double)u[p], scale[0]);
    const double wy = __dmul_rn((double)u[vol.V + p], scale[1]);
    const double wz = __dmul_rn((double)u[2 * vol.V + p], scale[2]);
    const double n2 = __dadd_rn(__dadd_rn(__dmul_rn(wx, wx), __dmul_rn(wy, wy)), __dmul_rn(wz, wz));
    const double n1 = __dsqrt_rn(n2);
    const float det = det_jacobian(t, p, x, y, z, vol);
    a.i[0] = 1;
    a.i[1] = !(det > 0.0f);
    a.f[0] = wx;
    a.f[1] = wy;
    a.f[2] = wz;
    a.f[3] = n1;
    a.f[4] = n2;
    a.f[5] = fmax(a.f[5], n1);
    if (det == det) {
        a.f[6] = (double)det;
        a.f[7] = (double)det;
        a.f[8] = (double)det;
    }
    return a;
}

// one value of one map: x^2 is formed in double and is exact
__device__ __forceinline__ SummaryAcc<StructureMapStats> structure_map_voxel(float v) {
    SummaryAcc<StructureMapStats> a = SummaryAcc<StructureMapStats>::identity();
    const bool finite = fabsf(v) <= 3.402823466e+38f;  // false for NaN and +-inf
    a.i[0] = finite;
    a.i[1] = !finite;
    if (finite) {
        const double x = (double)v;
        a.f[0] = x;
        a.f[1] = __dmul_rn(x, x);
        a.f[2] = x;
        a.f[3] = x;
    }
    return a;
}

// the LDS tables of a block: one per wavefront, [K][kInts] and [K][kFloats]
template <class T>
struct StructureTables {
    long long i[kStructureWaves][IRS_MAX_LABELS * T::kInts];
    double f[kStructureWaves][IRS_MAX_LABELS * T::kFloats];

    __device__ __forceinline__ void clear(int K) {
        for (int e = threadIdx.x; e < kStructureWaves * K * T::kInts; e += kBlock) i[e / (K * T::kInts)][e % (K * T::kInts)] = 0;
        for (int e = threadIdx.x; e < kStructureWaves * K * T::kFloats; e += kBlock) {
            const int c = e % T::kFloats;
            f[e / (K * T::kFloats)][e % (K * T::kFloats)] = T::kind(c) == Col::Sum ? 0.0 : T::kind(c) == Col::Max ? -INFINITY : INFINITY;
        }
        __syncthreads();
    }
};

// Every lane of the wavefront must reach the call (ballot + shuffle); a lane without a voxel, or whose voxel belongs to no
// structure, passes j = -1.  Per distinct j of the wavefront, lowest holding lane first: the butterfly over the 64 lanes, one
// level for all columns at a time, and one merge into the wavefront's table by lane 0.
template <class T>
__device__ __forceinline__ void structure_wave_fold(int j, const SummaryAcc<T>& a, StructureTables<T>& tab) {
    unsigned long long todo = __ballot(j >= 0);
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int jl = __shfl(j, leader, kWave);
        const bool mine = j == jl;
        SummaryAcc<T> r = mine ? a : SummaryAcc<T>::identity();
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            SummaryAcc<T> o;
#pragma unroll
            for (int c = 0; c < T::kInts; ++c) o.i[c] = __shfl_down(r.i[c], off, kWave);
#pragma unroll
            for (int c = 0; c < T::kFloats; ++c) o.f[c] = __shfl_down(r.f[c], off, kWave);
            r.merge(o);
        }
        if (lane == 0) {
            SummaryAcc<T> s = SummaryAcc<T>::load(tab.i[wid], tab.f[wid], jl);
            s.merge(r);
            s.store(tab.i[wid], tab.f[wid], jl);
        }
        todo &= ~__ballot(mine);
    }
}

// the four tables merged in wavefront order -> the block's partials: entry (row, j, block) of ipart / fpart, laid out
// [row][j][block][column] so that the rows of one (row, j) are contiguous for the second stage
template <class T>
__device__ __forceinline__ void structure_block_store(const StructureTables<T>& tab, int K, int64_t row, long long* __restrict__ ipart,
                                                      double* __restrict__ fpart) {
    __syncthreads();
    const int64_t nb = gridDim.x;
    for (int e = threadIdx.x; e < K * T::kInts; e += kBlock) {
        long long s = tab.i[0][e];
        for (int w = 1; w < kStructureWaves; ++w) s += tab.i[w][e];
        const int j = e / T::kInts, c = e - j * T::kInts;
        ipart[((row * K + j) * nb + blockIdx.x) * T::kInts + c] = s;
    }
    for (int e = threadIdx.x; e < K * T::kFloats; e += kBlock) {
        const int j = e / T::kFloats, c = e - j * T::kFloats;
        double s = tab.f[0][e];
        for (int w = 1; w < kStructureWaves; ++w)
            s = T::kind(c) == Col::Sum ? s + tab.f[w][e] : T::kind(c) == Col::Max ? fmax(s, tab.f[w][e]) : fmin(s, tab.f[w][e]);
        fpart[((row * K + j) * nb + blockIdx.x) * T::kFloats + c] = s;
    }
}

// second stage, one block per (structure, row): the nblocks partial rows folded as summary_reduce_kernel folds them (thread i
// takes blocks i, i + 256, ... in order, then the block reduction) -> ints / floats (rows, K, columns)
template <class T>
__global__ __launch_bounds__(kBlock) void structure_fold_kernel(const long long* __restrict__ ipart, const double* __restrict__ fpart,
                                                                int nblocks, int K, int64_t row0, long long* __restrict__ ints,
                                                                double* __restrict__ floats) {
    __shared__ SummaryAcc<T> smem[SummaryAcc<T>::kG];
    const int64_t rj = (row0 + blockIdx.y) * K + blockIdx.x;
    const long long* ip = ipart + rj * nblocks * T::kInts;
    const double* fp = fpart + rj * nblocks * T::kFloats;
    SummaryAcc<T> a = SummaryAcc<T>::identity();
    for (int b = threadIdx.x; b < nblocks; b += kBlock) a.merge(SummaryAcc<T>::load(ip, fp, b));
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ints, floats, rj);
}

}  // namespace irs
