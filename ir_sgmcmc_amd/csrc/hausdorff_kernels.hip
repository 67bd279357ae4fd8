// Hausdorff and percentile surface distances: exact order statistics of the squared contour distances that pass D of
// metric_kernels.hip kept in the box arrays (KEEP variant).
//
//  - keys: the float32 squared distances are non-negative, so their bit patterns order as unsigned integers.  Selection is
//    exact on the keys; the reported value is sqrt((double)key as float).
//  - per (pair, direction) the set is the box voxels whose membership byte has the source-contour bit; its size is the
//    count the ASD reduction wrote, so the ranks are formed on the device (hd_begin_kernel), in double, in the order
//    k = min(max((int64)ceil(q * (double)n / 100.0) - 1, 0), n - 1).
//  - MSB-first radix select, 8 bits per pass, 4 passes.  hd_hist_kernel: blocks (slice, pair x direction) stream the
//    membership bytes four at a time and load a key only at a contour voxel; 256-bin integer histograms in LDS, one per
//    rank whose prefix differs from the rank below (pass 0: one), flushed with integer global atomics.  hd_scan_kernel: a
//    wavefront per rank finds the bin that holds the rank and extends the prefix.  Integer counts only: the result does not
//    depend on the order of the atomics.
//  - the directed maximum does not come from the selection: hd_begin_kernel reduces the per-task maxima of pass D.
#include <algorithm>

#include "kernels.h"

namespace irs {
namespace {

constexpr int kQ = IRS_HAUSDORFF_MAX_PERCENTILES;
constexpr double kInfD = __builtin_huge_val();
constexpr long long kHdMinChunk = 4096;  // voxels of a slice at least: small boxes use few of the blocks of their row

// the rank whose histogram rank r shares: the lowest one with the same prefix (ranks ascend, so equal prefixes are adjacent)
__device__ __forceinline__ int hist_owner(const uint32_t* __restrict__ prefix, int r) {
    int o = r;
    while (o > 0 && prefix[o - 1] == prefix[r]) --o;
    return o;
}

// one block per (pair, direction): the directed maximum from the per-task maxima, the ranks, and +inf everywhere for a pair
// with an empty contour
__global__ __launch_bounds__(kBlock) void hd_begin_kernel(HdArgs a) {
    __shared__ uint32_t smax[kBlock / kWave];
    const int pd = blockIdx.x, p = pd >> 1, dir = pd & 1;
    const long long nA = a.counts[2 * p], nB = a.counts[2 * p + 1];
    const bool empty = nA == 0 || nB == 0;
    uint32_t m = 0u;
    for (int64_t t = a.plan[p].td + threadIdx.x; t < a.plan[p + 1].td; t += kBlock) m = max(m, a.maxpart[t * 2 + dir]);
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_down((int)m, off, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) smax[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w) m = max(m, smax[w]);
        a.hd[pd] = empty ? kInfD : sqrt((double)__uint_as_float(m));
    }
    if (threadIdx.x < a.Q) {
        const int r = threadIdx.x;
        const long long n = dir == 0 ? nA : nB;
        long long k = (long long)ceil(a.pct[r] * (double)n / 100.0) - 1;
        k = min(max(k, 0ll), n - 1);
        a.rank[pd * a.Q + r] = empty ? -1 : k;
        a.prefix[pd * a.Q + r] = 0u;
        a.hd_pct[((int64_t)r * a.P + p) * 2 + dir] = kInfD;  // stays for an empty contour; the last scan overwrites it
    }
}

// blocks (slice, pair x direction): histogram of the digit of `pass` over the keys whose higher bits equal a rank's prefix
__global__ __launch_bounds__(kBlock) void hd_hist_kernel(HdArgs a, int pass) {
    __shared__ uint32_t h[kQ][256];
    const int pd = blockIdx.y, p = pd >> 1, dir = pd & 1, Q = a.Q;
    if (a.rank[pd * Q] < 0) return;  // every rank of the pair is off together
    const SurfPair q = a.plan[p];
    const long long nvox = (long long)q.nz * q.ny * q.nx;
    const long long chunk = max((((nvox + a.slices - 1) / a.slices) + 3) & ~3ll, kHdMinChunk);
    const long long start = q.vox + blockIdx.x * chunk, end = min((long long)q.vox + nvox, start + chunk);
    if (start >= end) return;
    uint32_t pref[kQ];
    bool own[kQ];
#pragma unroll
    for (int r = 0; r < kQ; ++r) {
        pref[r] = r < Q ? a.prefix[pd * Q + r] : 0u;
        own[r] = r < Q && hist_owner(a.prefix + pd * Q, r) == r;
    }
#pragma unroll
    for (int r = 0; r < kQ; ++r) h[r][threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t src = dir == 0 ? 1u : 2u;
    const float* __restrict__ g = dir == 0 ? a.gB : a.gA;
    const uint32_t* __restrict__ memb4 = (const uint32_t*)a.memb;  // the array starts on a 256-byte boundary
    const int shift = 24 - 8 * pass;
    for (long long g4 = (start >> 2) + threadIdx.x; g4 < ((end + 3) >> 2); g4 += kBlock) {
        const uint32_t m4 = memb4[g4];
        if (!(m4 & (0x01010101u * src))) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long idx = g4 * 4 + j;
            if (!((m4 >> (8 * j)) & src) || idx < start || idx >= end) continue;
            const uint32_t key = __float_as_uint(g[idx]);
            const uint32_t hi = pass == 0 ? 0u : key >> (shift + 8);
            const uint32_t digit = (key >> shift) & 255u;
#pragma unroll
            for (int r = 0; r < kQ; ++r)
                if (own[r] && hi == pref[r]) atomicAdd(&h[r][digit], 1u);
        }
    }
    __syncthreads();
    uint32_t* out = a.hist + (((int64_t)pass * 2 * a.P + pd) * Q) * 256;
#pragma unroll
    for (int r = 0; r < kQ; ++r) {
        if (!own[r]) continue;
        const uint32_t v = h[r][threadIdx.x];
        if (v) atomicAdd(out + r * 256 + threadIdx.x, v);
    }
}

// one block per (pair, direction), a wavefront per rank: the bin of `pass` that holds the rank; the last pass writes the value
__global__ __launch_bounds__(kQ * kWave) void hd_scan_kernel(HdArgs a, int pass) {
    const int pd = blockIdx.x, p = pd >> 1, dir = pd & 1, Q = a.Q;
    if (a.rank[pd * Q] < 0) return;
    const int r = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int owner = r < Q ? hist_owner(a.prefix + pd * Q, r) : 0;
    __syncthreads();  // every wavefront has read the prefixes of the ranks below before one is extended
    if (r >= Q) return;
    const long long k = a.rank[pd * Q + r];
    const uint32_t* row = a.hist + (((int64_t)pass * 2 * a.P + pd) * Q + owner) * 256;
    const uint4 c = ((const uint4*)row)[lane];  // bins 4 lane .. 4 lane + 3
    const uint32_t tot = c.x + c.y + c.z + c.w;
    uint32_t incl = tot;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off, kWave);
        if (lane >= off) incl += up;
    }
    const long long before = (long long)(incl - tot);
    if (k >= before && k < before + tot) {  // one lane: the counts of the prefix sum to more than k
        const uint32_t cc[4] = {c.x, c.y, c.z, c.w};
        long long lo = before;
        int b = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (b == j && k >= lo + cc[j]) {
                lo += cc[j];
                b = j + 1;
            }
        const uint32_t prefix = (a.prefix[pd * Q + r] << 8) | (uint32_t)(4 * lane + b);
        a.prefix[pd * Q + r] = prefix;
        a.rank[pd * Q + r] = k - lo;
        if (pass == 3) a.hd_pct[((int64_t)r * a.P + p) * 2 + dir] = sqrt((double)__uint_as_float(prefix));
    }
}

}  // namespace

void launch_hausdorff_select(const HdArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(hd_begin_kernel, dim3(2 * a.P), dim3(kBlock), 0, st, a);
    if (a.Q == 0) return;
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(hd_hist_kernel, dim3(a.slices, 2 * a.P), dim3(kBlock), 0, st, a, pass);
        hipLaunchKernelGGL(hd_scan_kernel, dim3(2 * a.P), dim3(kQ * kWave), 0, st, a, pass);
    }
}

}  // namespace irs
