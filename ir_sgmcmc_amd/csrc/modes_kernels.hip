// Posterior principal modes (absent in the reference; DESIGN.md section 6, "Displacement modes"): the recorded displacements
// are kept on the device, store (cap,3,V) float32, and everything the snapshot PCA needs comes from their Gram matrix.
//
//  - gram rows: one call per recorded step.  modes_gram_partial_kernel runs on a grid of (voxel chunks) x (tiles of kGramJ
//    stored records) x (pairs of new records).  A thread walks its grid-stride voxels in order; per voxel it loads the mask
//    byte and the three channels of its two new records once and the kGramJ stored records of the tile, and folds the
//    3 x kGramJ x 2 products into double accumulators (modes_device.h: every product exact).  The block reduces them in a fixed
//    order (lanes by the shuffle butterfly, then the wavefronts in order) and stores one row of partials.
//    modes_gram_finish_kernel adds the rows of the chunks in order and writes G[c][i][j] and G[c][j][i] from the one value.
//    The number of chunks depends on V only, so the order of every sum depends on (D, H, W) and the constants below, never on
//    how many records are stored.  No atomics.
//  - project: one launch, one voxel per thread, the channels one after the other: a thread streams the n records of a channel
//    once and keeps the M mode sums, the sum and the sum of squares in double (M + 2 accumulators live at a time, not 3 M + 6:
//    the channels share no term but the two scalars of the explained ratio).  The coefficients are read at wave-uniform
//    addresses.
#include <algorithm>

#include "kernels.h"
#include "modes_device.h"

namespace irs {
namespace {

constexpr int kGramJ = 8;            // stored records per tile
constexpr int kGramPair = 2;         // new records per block
constexpr int kGramMaxChunks = 256;  // voxel chunks (rows of partials)
constexpr int kGramAcc = 3 * kGramJ * kGramPair;

int gram_chunks(int64_t V) { return (int)std::min<int64_t>((V + kBlock - 1) / kBlock, kGramMaxChunks); }
int gram_padded(int n) { return (n + kGramJ - 1) / kGramJ * kGramJ; }

// partials (chunks, n_new, 3, padded) double: [chunk][new record][channel][stored record]
__global__ __launch_bounds__(kBlock) void modes_gram_partial_kernel(const float* __restrict__ store, int n_before, int n_new, int64_t V,
                                                                    const uint8_t* __restrict__ mask, int padded,
                                                                    double* __restrict__ partials) {
    __shared__ double smem[kGramAcc * (kBlock / kWave)];
    const int n = n_before + n_new;
    const int j0 = blockIdx.y * kGramJ;
    const int a0 = blockIdx.z * kGramPair, a1 = min(a0 + 1, n_new - 1);  // an odd count: the last pair is one record twice
    if (j0 > n_before + a1) return;                                       // nothing of this tile is at or below the diagonal
    const float* xa0 = store + (int64_t)(n_before + a0) * 3 * V;
    const float* xa1 = store + (int64_t)(n_before + a1) * 3 * V;
    double acc[kGramAcc];
#pragma unroll
    for (int k = 0; k < kGramAcc; ++k) acc[k] = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        if (mask && !mask[v]) continue;
        float a[2][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[0][c] = xa0[c * V + v];
            a[1][c] = xa1[c * V + v];
        }
#pragma unroll
        for (int jj = 0; jj < kGramJ; ++jj) {
            const int j = min(j0 + jj, n - 1);  // past the last record: a copy of it, never written
            const float* xs = store + (int64_t)j * 3 * V + v;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float s = xs[c * V];
                acc[(0 * 3 + c) * kGramJ + jj] = modes_gram_term(acc[(0 * 3 + c) * kGramJ + jj], a[0][c], s);
                acc[(1 * 3 + c) * kGramJ + jj] = modes_gram_term(acc[(1 * 3 + c) * kGramJ + jj], a[1][c], s);
            }
        }
    }
    // block_sum's additions in block_sum's order, kGramJ values at a time: all 48 at once would need 48 more doubles live
    // (194 VGPRs against 128, two waves per SIMD against four)
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
    for (int g = 0; g < kGramAcc; g += kGramJ) {
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            double t[kGramJ];
#pragma unroll
            for (int k = 0; k < kGramJ; ++k) t[k] = __shfl_down(acc[g + k], off, kWave);
#pragma unroll
            for (int k = 0; k < kGramJ; ++k) acc[g + k] += t[k];
        }
#pragma unroll
        for (int k = 0; k < kGramJ; ++k)
            if (lane == 0) smem[(g + k) * (kBlock / kWave) + wid] = acc[g + k];
    }
    __syncthreads();
    if (threadIdx.x < kGramAcc) {  // thread k: value k of the block, the wavefronts in order
        const int k = threadIdx.x, p = k / (3 * kGramJ), c = k / kGramJ % 3, jj = k % kGramJ, ai = a0 + p;
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) s += smem[k * (kBlock / kWave) + w];
        if (ai < n_new) partials[(((int64_t)blockIdx.x * n_new + ai) * 3 + c) * padded + j0 + jj] = s;
    }
}

// one thread per (new record, channel, stored record at or below the diagonal): the chunks in order, both triangles
__global__ __launch_bounds__(kBlock) void modes_gram_finish_kernel(const double* __restrict__ partials, int chunks, int n_before, int n_new,
                                                                   int padded, int cap, double* __restrict__ gram) {
    const int n = n_before + n_new;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_new * 3 * n) return;
    const int j = t % n, c = (t / n) % 3, ai = t / (3 * n), i = n_before + ai;
    if (j > i) return;
    double s = 0.0;
    for (int b = 0; b < chunks; ++b) s += partials[(((int64_t)b * n_new + ai) * 3 + c) * padded + j];
    gram[((int64_t)c * cap + i) * cap + j] = s;
    gram[((int64_t)c * cap + j) * cap + i] = s;
}

struct ModesScale {
    double s2[3];  // the squared channel scales
};

// store (.,3,V) float32, coeff (M,n) double -> mean (3,V), modes (M,3,V), explained (V) float32.  MP: M rounded up to a
// power of two -- the accumulators are registers, the modes beyond M are never touched.
template <int MP>
__global__ __launch_bounds__(kBlock) void modes_project_kernel(const float* __restrict__ store, int n, int64_t V,
                                                               const double* __restrict__ coeff, int M, ModesScale scale,
                                                               float* __restrict__ mean, float* __restrict__ modes,
                                                               float* __restrict__ explained) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    double num = 0.0, den = 0.0;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        double acc[MP];
#pragma unroll
        for (int m = 0; m < MP; ++m) acc[m] = 0.0;
        double sum = 0.0, sumsq = 0.0;
        const float* x = store + c * V + v;
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const float xi = x[(int64_t)i * 3 * V];
            sum = modes_add(sum, (double)xi);
            sumsq = modes_gram_term(sumsq, xi, xi);
#pragma unroll
            for (int m = 0; m < MP; ++m)
                if (m < M) acc[m] = modes_axpy(acc[m], coeff[(int64_t)m * n + i], xi);
        }
        mean[c * V + v] = (float)(sum / (double)n);
        double q = 0.0;
#pragma unroll
        for (int m = 0; m < MP; ++m)
            if (m < M) {
                modes[((int64_t)m * 3 + c) * V + v] = (float)acc[m];
                q += acc[m] * acc[m];
            }
        num += scale.s2[c] * q;
        if (n > 1) den += scale.s2[c] * modes_variance(sum, sumsq, n);
    }
    explained[v] = modes_explained(num, den, n);
}

}  // namespace

size_t modes_gram_workspace_bytes(int64_t V, int n_new) {
    return (size_t)gram_chunks(V) * n_new * 3 * gram_padded(IRS_MODES_MAX_RECORDS) * sizeof(double);
}

void launch_modes_gram_rows(const float* store, int cap, int n_before, int n_new, int64_t V, const uint8_t* mask, double* gram, void* ws,
                            hipStream_t st) {
    const int n = n_before + n_new, chunks = gram_chunks(V), padded = gram_padded(n);
    double* partials = (double*)ws;
    const dim3 grid((unsigned)chunks, (unsigned)(padded / kGramJ), (unsigned)((n_new + kGramPair - 1) / kGramPair));
    hipLaunchKernelGGL(modes_gram_partial_kernel, grid, dim3(kBlock), 0, st, store, n_before, n_new, V, mask, padded, partials);
    hipLaunchKernelGGL(modes_gram_finish_kernel, dim3((unsigned)((n_new * 3 * n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, partials,
                       chunks, n_before, n_new, padded, cap, gram);
}

void launch_modes_project(const float* store, int n, int64_t V, const double* coeff, int M, const double* scale, float* mean, float* modes,
                          float* explained, hipStream_t st) {
    const ModesScale sc{{scale[0] * scale[0], scale[1] * scale[1], scale[2] * scale[2]}};
    const dim3 grid((unsigned)((V + kBlock - 1) / kBlock));
#define IRS_MODES_PROJECT(MP) \
    hipLaunchKernelGGL(modes_project_kernel<MP>, grid, dim3(kBlock), 0, st, store, n, V, coeff, M, sc, mean, modes, explained)
    if (M <= 1) IRS_MODES_PROJECT(1);
    else if (M <= 2) IRS_MODES_PROJECT(2);
    else if (M <= 4) IRS_MODES_PROJECT(4);
    else if (M <= 8) IRS_MODES_PROJECT(8);
    else IRS_MODES_PROJECT(16);
#undef IRS_MODES_PROJECT
}

}  // namespace irs
