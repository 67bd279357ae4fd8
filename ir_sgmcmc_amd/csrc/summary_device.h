// The masked summary of a per-voxel posterior finalize (jacobian / covariance / quantile_kernels.hip), reduced in two stages.
//
// A family describes its columns in a traits type T: T::kInts int64 sums, then T::kFloats doubles, each a sum, a maximum or
// a minimum by the constexpr T::kind(j).  The finalize kernel keeps a SummaryAcc<T> in registers over its grid-stride loop,
// reduces it over the block (lanes by the shuffle butterfly, then the wavefronts in order) and stores one row of partials per
// block; summary_reduce_kernel<T>, one block, folds the rows: thread i takes blocks i, i + 256, ... in order, then the same
// block reduction.  The grids depend on the volume only and every merge has a fixed order, so two identical call sequences
// are bit-identical.  A maximum nothing entered stays -inf, a minimum +inf; fmax / fmin must never be fed a NaN.
#pragma once
#include <algorithm>

#include "common.h"

namespace irs {

enum class Col { Sum, Max, Min };

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, kWave));
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, kWave));
    return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

template <class T>
struct SummaryAcc {
    static constexpr int kG = kBlock / kWave;  // rows of LDS block_reduce needs
    long long i[T::kInts];
    double f[T::kFloats];

    static __device__ __forceinline__ SummaryAcc identity() {
        SummaryAcc a;
#pragma unroll
        for (int j = 0; j < T::kInts; ++j) a.i[j] = 0;
#pragma unroll
        for (int j = 0; j < T::kFloats; ++j)
            a.f[j] = T::kind(j) == Col::Sum ? 0.0 : T::kind(j) == Col::Max ? -INFINITY : INFINITY;
        return a;
    }
    __device__ __forceinline__ void merge(const SummaryAcc& b) {
#pragma unroll
        for (int j = 0; j < T::kInts; ++j) i[j] += b.i[j];
#pragma unroll
        for (int j = 0; j < T::kFloats; ++j)
            f[j] = T::kind(j) == Col::Sum ? f[j] + b.f[j] : T::kind(j) == Col::Max ? fmax(f[j], b.f[j]) : fmin(f[j], b.f[j]);
    }
    // thread 0 ends with the block's accumulator
    __device__ __forceinline__ void block_reduce(SummaryAcc* smem) {
#pragma unroll
        for (int j = 0; j < T::kInts; ++j) i[j] = wave_sum_ll(i[j]);
#pragma unroll
        for (int j = 0; j < T::kFloats; ++j)
            f[j] = T::kind(j) == Col::Sum ? wave_sum(f[j]) : T::kind(j) == Col::Max ? wave_max(f[j]) : wave_min(f[j]);
        const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
        if (lane == 0) smem[wid] = *this;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 1; w < kG; ++w) merge(smem[w]);
    }
    // row `row` of the partials (row 0 of isummary / fsummary: the summary itself)
    __device__ __forceinline__ void store(long long* ip, double* fp, int64_t row = 0) const {
#pragma unroll
        for (int j = 0; j < T::kInts; ++j) ip[row * T::kInts + j] = i[j];
#pragma unroll
        for (int j = 0; j < T::kFloats; ++j) fp[row * T::kFloats + j] = f[j];
    }
    static __device__ __forceinline__ SummaryAcc load(const long long* ip, const double* fp, int64_t row) {
        SummaryAcc a;
#pragma unroll
        for (int j = 0; j < T::kInts; ++j) a.i[j] = ip[row * T::kInts + j];
#pragma unroll
        for (int j = 0; j < T::kFloats; ++j) a.f[j] = fp[row * T::kFloats + j];
        return a;
    }
};

template <class T>
__global__ __launch_bounds__(kBlock) void summary_reduce_kernel(const long long* __restrict__ ipart, const double* __restrict__ fpart,
                                                                int nblocks, long long* __restrict__ isummary,
                                                                double* __restrict__ fsummary) {
    __shared__ SummaryAcc<T> smem[SummaryAcc<T>::kG];
    SummaryAcc<T> a = SummaryAcc<T>::identity();
    for (int b = threadIdx.x; b < nblocks; b += kBlock) a.merge(SummaryAcc<T>::load(ipart, fpart, b));
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(isummary, fsummary);
}

// host: the finalize grid for V voxels and its rows of partials in the family's workspace of ws_bytes (IRS_*_WS_BYTES: one
// row per block, which caps the grid), and the second stage over them
template <class T>
struct SummaryPartials {
    int blocks;
    long long* ipart;
    double* fpart;
    SummaryPartials(int64_t V, void* ws, int ws_bytes)
        : blocks((int)std::min<int64_t>((V + kBlock - 1) / kBlock, ws_bytes / (T::kInts + T::kFloats) / 8)),
          ipart((long long*)ws),
          fpart((double*)(ipart + (size_t)T::kInts * blocks)) {}
    void reduce(long long* isummary, double* fsummary, hipStream_t st) const {
        hipLaunchKernelGGL(summary_reduce_kernel<T>, dim3(1), dim3(kBlock), 0, st, ipart, fpart, blocks, isummary, fsummary);
    }
};

}  // namespace irs
