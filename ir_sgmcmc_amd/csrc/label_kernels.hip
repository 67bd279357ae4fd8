// Posterior label maps of the propagated segmentation (absent in the reference): per-voxel counts of every structure over the
// recorded warps, and at the end the entropy / MAP maps and the whole-volume sums behind soft Dice, Dice of the MAP, volume
// spread and calibration.
//
//  - update: one launch per recorded step for all C chains.  A grid-stride stream over voxels, 8 per thread (one 16-byte load
//    of each chain's int16 map) when the volume allows it, one otherwise.  Each thread owns its voxels, so the count
//    increments are plain read-modify-writes (16 bytes when four neighbours carry the same structure).  The per-record volumes
//    are counted per block in LDS, one integer add per distinct structure of a wavefront (ballot + popcount); the block
//    partials (C x K int32) go to the workspace and one block reduces them and folds the Welford update in chain order.
//  - finalize: one voxel per thread reads its K counts, the fixed segmentation and the mask, writes the entropy and the MAP
//    label, and adds its non-zero contributions to the per-structure sums with LDS integer atomics (exact, so their order
//    does not matter).  The entropy sum and max over the mask stay in registers and are reduced in fixed order.  Per-block
//    partials are reduced, column by column, in block order.  The grids depend on the volume only, so two identical call
//    sequences are bit-identical.
#include <algorithm>

#include "label_device.h"

namespace irs {
namespace {

constexpr int kLabelMaxBlocks = 1024;  // 256 CUs x 4 blocks of 4 wavefronts
constexpr int kLabelCols = 6 + 3 * IRS_LABEL_BINS;  // S0 .. S5, then per bin: pairs, sum of c, sum of y

__device__ __forceinline__ void count_one(int32_t* __restrict__ counts, int j, int64_t V, int64_t v) {
    if (j >= 0) counts[(int64_t)j * V + v] += 1;
}

// four neighbours v0 .. v0 + 3 (v0 % 4 == 0): one 16-byte read-modify-write when they carry the same structure
__device__ __forceinline__ void count_four(int32_t* __restrict__ counts, const int (&j)[8], int s, int64_t V, int64_t v0) {
    if (j[s] == j[s + 1] && j[s] == j[s + 2] && j[s] == j[s + 3]) {
        if (j[s] >= 0) {
            int4* p = reinterpret_cast<int4*>(counts + (int64_t)j[s] * V + v0);
            int4 c = *p;
            c.x += 1;
            c.y += 1;
            c.z += 1;
            c.w += 1;
            *p = c;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) count_one(counts, j[s + t], V, v0 + t);
    }
}

// seg (C,V) int16, counts (K,V) int32; partials: C x K int32 per block.  VEC: V % 8 == 0 and 16-byte aligned bases.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void label_update_kernel(const int16_t* __restrict__ seg, int C, int64_t V, SurfLabels lab,
                                                              int K, int32_t* __restrict__ counts, int32_t* __restrict__ partials) {
    __shared__ int vol[IRS_MAX_CHAINS * IRS_MAX_LABELS];
    const int CK = C * K;
    for (int i = threadIdx.x; i < CK; i += kBlock) vol[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t units = VEC ? V >> 3 : V;
    for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < units; u += stride) {
        for (int c = 0; c < C; ++c) {
            if (VEC) {
                const int4 raw = reinterpret_cast<const int4*>(seg + (int64_t)c * V)[u];
                const int w[4] = {raw.x, raw.y, raw.z, raw.w};
                int j[8];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    j[2 * s] = structure_of((int16_t)(w[s] & 0xFFFF), lab, K);
                    j[2 * s + 1] = structure_of((int16_t)((uint32_t)w[s] >> 16), lab, K);
                }
                count_four(counts, j, 0, V, u << 3);
                count_four(counts, j, 4, V, (u << 3) + 4);
#pragma unroll
                for (int s = 0; s < 8; ++s) wave_count(j[s], vol + c * K);
            } else {
                const int j = structure_of(seg[(int64_t)c * V + u], lab, K);
                count_one(counts, j, V, u);
                wave_count(j, vol + c * K);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CK; i += kBlock) partials[(int64_t)blockIdx.x * CK + i] = vol[i];
}

// one block: the per-record volumes of this step (block partials summed column by column, four row groups, in block
// order), then per structure the Welford fold of the C records in chain order, k = records_before + c + 1
__global__ __launch_bounds__(kBlock) void label_volume_fold_kernel(const int32_t* __restrict__ partials, int nblocks, int C,
                                                                   int K, double* __restrict__ volume, int records_before) {
    __shared__ long long tot[IRS_MAX_CHAINS * IRS_MAX_LABELS];
    __shared__ long long part[kBlock / kWave][kWave];
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const int CK = C * K;
    for (int c0 = 0; c0 < CK; c0 += kWave) {
        const int p = c0 + lane;
        long long s = 0;
        if (p < CK)
            for (int b = wid; b < nblocks; b += kBlock / kWave) s += partials[(int64_t)b * CK + p];
        part[wid][lane] = s;
        __syncthreads();
        if (wid == 0 && p < CK) {
            long long t = 0;
            for (int w = 0; w < kBlock / kWave; ++w) t += part[w][lane];
            tot[p] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x < K) {
        const int j = threadIdx.x;
        double mean = volume[2 * j], m2 = volume[2 * j + 1];
        for (int c = 0; c < C; ++c) {
            const long long k = (long long)records_before + c + 1;
            const double x = (double)tot[c * K + j];
            if (k == 1) {  // the first record overwrites whatever the state held
                mean = x;
                m2 = 0.0;
                continue;
            }
            const double d = x - mean;
            mean += d / (double)k;
            m2 += d * (x - mean);
        }
        volume[2 * j] = mean;
        volume[2 * j + 1] = m2;
    }
}

__device__ __forceinline__ void lds_add(unsigned long long* s, long long x) { atomicAdd(s, (unsigned long long)x); }

// c * (ln n - ln c), c >= 1: a class's share of n H (a class holding all n records adds exactly 0)
__device__ __forceinline__ double entropy_term(int64_t c, double ln_n) { return (double)c * (ln_n - log((double)c)); }

// counts (K,V) int32; partials: K x kLabelCols int64 per block; dpartials: 4 doubles per block {voxels in the mask, sum of
// the stored entropy over them, its max, voxels with sum_j c_j > n}
__global__ __launch_bounds__(kBlock) void label_finalize_kernel(const int32_t* __restrict__ counts, int K, int64_t V, int n,
                                                                SurfLabels lab, const int16_t* __restrict__ seg_fixed,
                                                                const uint8_t* __restrict__ mask, float* __restrict__ entropy,
                                                                int16_t* __restrict__ map_label, long long* __restrict__ partials,
                                                                double* __restrict__ dpartials) {
    __shared__ unsigned long long s[IRS_MAX_LABELS * kLabelCols];
    __shared__ double smem[3 * (kBlock / kWave)];
    const int KC = K * kLabelCols;
    for (int i = threadIdx.x; i < KC; i += kBlock) s[i] = 0;
    __syncthreads();
    const double ln_n = log((double)n), inv_n = 1.0 / (double)n;
    double vox = 0.0, hsum = 0.0, hmax = 0.0, bad = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        const int f = seg_fixed[v];
        int64_t total = 0;
        double h = 0.0;
        int best = 0, best_j = -1;  // first structure with the largest count
        for (int j0 = 0; j0 < K; j0 += 8) {
            int cj[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) cj[t] = j0 + t < K ? counts[(int64_t)(j0 + t) * V + v] : 0;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int j = j0 + t;
                if (j >= K) break;
                const int c = cj[t];
                const bool y = f == lab.v[j];
                total += c;
                if (c > best) {
                    best = c;
                    best_j = j;
                }
                unsigned long long* sj = s + j * kLabelCols;
                if (c > 0) {
                    h += entropy_term(c, ln_n);
                    lds_add(sj + 1, c);
                    if (y) lds_add(sj + 2, c);
                    if (c < n) lds_add(sj + 5, 1);
                }
                if (y) lds_add(sj + 0, 1);
                if (c > 0 || y) {
                    // clamped both ways: c > n (a wrong n, counted below) or corrupt counts never leave the bins
                    const int b = (int)std::max<int64_t>(0, std::min<int64_t>((int64_t)c * IRS_LABEL_BINS / n, IRS_LABEL_BINS - 1));
                    unsigned long long* sb = sj + 6 + 3 * b;
                    lds_add(sb, 1);
                    if (c > 0) lds_add(sb + 1, c);
                    if (y) lds_add(sb + 2, 1);
                }
            }
        }
        const int64_t other = (int64_t)n - total;
        if (other < 0) bad += 1.0;  // more records than n: n is not the number of recorded maps
        if (other > 0) h += entropy_term(other, ln_n);
        const int mj = other >= best ? -1 : best_j;  // ties go to "other", then to the first structure
        if (mj >= 0) {
            unsigned long long* sj = s + mj * kLabelCols;
            lds_add(sj + 3, 1);
            if (f == lab.v[mj]) lds_add(sj + 4, 1);
        }
        const float hf = (float)(h * inv_n);
        entropy[v] = hf;
        map_label[v] = (int16_t)(mj >= 0 ? lab.v[mj] : 0);
        if (!mask || mask[v]) {
            vox += 1.0;
            hsum += (double)hf;
            hmax = fmax(hmax, (double)hf);
        }
    }
    double acc[3] = {vox, hsum, bad};
    block_sum<3>(acc, smem);
    __syncthreads();  // block_sum's thread 0 reads smem after its barrier; the max below reuses it
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) hmax = fmax(hmax, __shfl_down(hmax, off, kWave));
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    if (lane == 0) smem[wid] = hmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; ++w) hmax = fmax(hmax, smem[w]);
        double* d = dpartials + (int64_t)blockIdx.x * 4;
        d[0] = acc[0];
        d[1] = acc[1];
        d[2] = hmax;
        d[3] = acc[2];
    }
    for (int i = threadIdx.x; i < KC; i += kBlock) partials[(int64_t)blockIdx.x * KC + i] = (long long)s[i];
}

// the per-block partials of the finalize, 64 columns per block: four row groups (one per wavefront) add their blocks in
// order, then the groups in order.  Block gridDim.x - 1 reduces the four doubles the same way (the max as a max).
__global__ __launch_bounds__(kBlock) void label_summary_reduce_kernel(const long long* __restrict__ partials,
                                                                      const double* __restrict__ dpartials, int nblocks, int KC,
                                                                      long long* __restrict__ summary,
                                                                      double* __restrict__ mask_summary) {
    constexpr int G = kBlock / kWave;
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ double dpart[G][4];
        double a = 0.0;  // the entropy is >= 0: 0 starts the max as well
        if (lane < 4)
            for (int b = wid; b < nblocks; b += G) {
                const double x = dpartials[(int64_t)b * 4 + lane];
                a = lane == 2 ? fmax(a, x) : a + x;
            }
        if (lane < 4) dpart[wid][lane] = a;
        __syncthreads();
        if (threadIdx.x < 4) {
            double t = dpart[0][threadIdx.x];
            for (int w = 1; w < G; ++w) t = threadIdx.x == 2 ? fmax(t, dpart[w][threadIdx.x]) : t + dpart[w][threadIdx.x];
            mask_summary[threadIdx.x] = t;
        }
        return;
    }
    __shared__ long long part[G][kWave];
    const int p = blockIdx.x * kWave + lane;
    long long a = 0;
    if (p < KC)
        for (int b = wid; b < nblocks; b += G) a += partials[(int64_t)b * KC + p];
    part[wid][lane] = a;
    __syncthreads();
    if (wid == 0 && p < KC) {
        long long t = 0;
        for (int w = 0; w < G; ++w) t += part[w][lane];
        summary[p] = t;
    }
}

}  // namespace

int label_finalize_blocks(int64_t V) { return (int)std::min<int64_t>((V + kBlock - 1) / kBlock, kLabelMaxBlocks); }

// the scalar update launches one voxel per thread, the vector one eight: the scalar grid is the larger
int label_update_partials_blocks(int64_t V) { return label_finalize_blocks(V); }

static int label_update_blocks(int64_t V, bool vec) {
    return vec ? (int)std::min<int64_t>((V / 8 + kBlock - 1) / kBlock, kLabelMaxBlocks) : label_finalize_blocks(V);
}

void launch_label_update(const int16_t* seg, int C, int64_t V, const SurfLabels& lab, int K, int32_t* counts, double* volume,
                         int records_before, int32_t* partials, hipStream_t st) {
    const bool vec = (V & 7) == 0 && (((uintptr_t)seg | (uintptr_t)counts) & 15) == 0;
    const int blocks = label_update_blocks(V, vec);
    if (vec)
        hipLaunchKernelGGL(label_update_kernel<true>, dim3(blocks), dim3(kBlock), 0, st, seg, C, V, lab, K, counts, partials);
    else
        hipLaunchKernelGGL(label_update_kernel<false>, dim3(blocks), dim3(kBlock), 0, st, seg, C, V, lab, K, counts, partials);
    launch_label_volume_fold(partials, blocks, C, K, volume, records_before, st);
}

void launch_label_volume_fold(const int32_t* partials, int nblocks, int C, int K, double* volume, int records_before, hipStream_t st) {
    hipLaunchKernelGGL(label_volume_fold_kernel, dim3(1), dim3(kBlock), 0, st, partials, nblocks, C, K, volume, records_before);
}

void launch_label_finalize(const int32_t* counts, int K, int64_t V, int n, const SurfLabels& lab, const int16_t* seg_fixed,
                           const uint8_t* mask, float* entropy, int16_t* map_label, long long* summary, double* mask_summary,
                           long long* partials, double* dpartials, hipStream_t st) {
    const int blocks = label_finalize_blocks(V);
    const int KC = K * kLabelCols;
    hipLaunchKernelGGL(label_finalize_kernel, dim3(blocks), dim3(kBlock), 0, st, counts, K, V, n, lab, seg_fixed, mask, entropy,
                       map_label, partials, dpartials);
    hipLaunchKernelGGL(label_summary_reduce_kernel, dim3((KC + kWave - 1) / kWave + 1), dim3(kBlock), 0, st, partials, dpartials,
                       blocks, KC, summary, mask_summary);
}

}  // namespace irs
