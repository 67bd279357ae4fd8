// Intensity similarity of the fixed image and a (warped) moving image (absent in the reference, which reports only its loss
// terms and segmentation metrics): per chain the joint intensity histogram and the moment sums in ONE pass
// over the two volumes, then the entropies, MI / NMI, MSE and the global NCC.
//
//  - accumulate: one launch for all chains, blockIdx.y the chain.  A grid-stride stream over the chain's voxels; each thread
//    reads fixed, moving and mask once (9 bytes per voxel and chain), four voxels per 16-byte load when V % 4 == 0 and the bases
//    are aligned (the base of chain c is c V floats), one otherwise.  A voxel takes part when the mask is set (or absent) and
//    both intensities are finite.  Binning in fp32: t = (x - lo) * inv_w -- a difference, then a product: nothing to contract --
//    b = min(B - 1, max(0, floor(t))); outside [lo, hi] counts as clipped.  The joint bin goes to a per-block B x B uint32
//    histogram in LDS (64 KB at B = 128; the block reduction reuses its first bytes once the histogram has left); the three
//    integer counts and the six double sums stay in registers (SummaryAcc, summary_device.h).  One LDS address hit by all 64
//    lanes serialises (a constant region: background, saturation): when every voxel a wavefront adds in one step falls into
//    ONE joint bin, its first lane adds their number instead -- two ballots and a v_readlane, still one LDS instruction per
//    step (the switch similarity_aggregate; 0: plain atomics always).  The ballot-and-leader LOOP of label_kernels.hip's
//    wave_count was measured and dropped: its ds_bpermute and second LDS add per leader cost more on smooth and on white-noise
//    images than the conflicts they save.  At the end the non-zero cells go to the global int32
//    histogram with integer atomics -- exact, so their order does not matter -- and one row of partials per block to the
//    workspace.
//  - finish: one block of 1024 threads per chain stages the chain's histogram in LDS, folds the chain's partial rows (thread
//    i row i, then the block reduction: lanes by the shuffle butterfly, the wavefronts in order), forms the row
//    and column sums from LDS without atomics, sums the p ln p terms in double in a fixed order and writes the
//    IRS_SIMILARITY_STATS doubles.
// Two identical call sequences are bit-identical: integer histogram, fixed-order double sums, grids that depend on (V, C) only.
#include <algorithm>

#include "histogram_device.h"
#include "kernels.h"
#include "summary_device.h"

namespace irs {
namespace {

// integer sums {voxels taking part, masked voxels with a non-finite intensity, voxels with a clipped intensity}; doubles
// {sum (f - m)^2, sum f, sum m, sum f^2, sum m^2, sum f m}
struct SimSummary {
    static constexpr int kInts = 3, kFloats = 6;
    static constexpr Col kind(int) { return Col::Sum; }
};
using SimAcc = SummaryAcc<SimSummary>;

constexpr int kSimCols = SimSummary::kInts + SimSummary::kFloats;

// the block's accumulator in thread 0.  The nine columns go through block_sum TOGETHER -- SummaryAcc::block_reduce takes them
// one by one, nine chains of six dependent shuffles at the tail of every block -- the counts as doubles: below 2^30, exact.
// smem: kSimCols * NW doubles, NW the wavefronts of the block
template <int NW = kBlock / kWave>
__device__ __forceinline__ void sim_block_reduce(SimAcc& a, double* smem) {
    double v[kSimCols];
#pragma unroll
    for (int j = 0; j < SimSummary::kInts; ++j) v[j] = (double)a.i[j];
#pragma unroll
    for (int j = 0; j < SimSummary::kFloats; ++j) v[SimSummary::kInts + j] = a.f[j];
    block_sum<kSimCols, NW>(v, smem);
#pragma unroll
    for (int j = 0; j < SimSummary::kInts; ++j) a.i[j] = (long long)v[j];
#pragma unroll
    for (int j = 0; j < SimSummary::kFloats; ++j) a.f[j] = v[SimSummary::kInts + j];
}

constexpr int kSimMaxBlocks = IRS_SIMILARITY_MAX_BLOCKS;  // all chains together: 256 CUs x 4 blocks of 4 wavefronts

struct SimVoxel {
    bool take;
    int cell;
};

// one voxel into the register sums; -> whether it takes part and its joint bin
__device__ __forceinline__ SimVoxel sim_voxel(float f, float m, bool masked, const SimBins& bn, SimAcc& a) {
    const bool finite = isfinite(f) && isfinite(m);
    const bool take = masked && finite;
    a.i[1] += masked && !finite;
    const float last = (float)(bn.bins - 1);
    const int bf = hist_bin(f, bn.f_lo, bn.f_inv, last), bm = hist_bin(m, bn.m_lo, bn.m_inv, last);
    if (take) {
        const double df = (double)f, dm = (double)m, d = df - dm;
        a.i[0] += 1;
        a.i[2] += f < bn.f_lo || f > bn.f_hi || m < bn.m_lo || m > bn.m_hi;
        a.f[0] += d * d;
        a.f[1] += df;
        a.f[2] += dm;
        a.f[3] += df * df;
        a.f[4] += dm * dm;
        a.f[5] += df * dm;
    }
    return {take, take ? bf * bn.bins + bm : 0};
}

// fixed (1 or C,V) with fixed_stride 0 or V; moving (C,V); mask (V) or nullptr; hist (C,B,B), zero on entry; row blockIdx.x of
// the chain's partials.  VEC: V % 4 == 0, fixed / moving 16-byte and mask 4-byte aligned.  Dynamic LDS: B * B * 4 bytes, at
// least kSimCols * (kBlock / kWave) doubles.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void similarity_accumulate_kernel(const float* __restrict__ fixed, int64_t fixed_stride,
                                                                       const float* __restrict__ moving,
                                                                       const uint8_t* __restrict__ mask, int64_t V, SimBins bn,
                                                                       bool aggregate, int32_t* __restrict__ hist,
                                                                       long long* __restrict__ ipart, double* __restrict__ fpart) {
    extern __shared__ __align__(16) unsigned char sim_lds[];
    uint32_t* h = reinterpret_cast<uint32_t*>(sim_lds);
    const int cells = bn.bins * bn.bins;
    for (int i = threadIdx.x; i < cells; i += kBlock) h[i] = 0;
    __syncthreads();

    const int chain = blockIdx.y;
    const float* f = fixed + (int64_t)chain * fixed_stride;
    const float* m = moving + (int64_t)chain * V;
    SimAcc a = SimAcc::identity();
    const int64_t units = VEC ? V >> 2 : V;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // the trip count is the wavefront's: the ballots of hist_add see every lane
    for (int64_t u0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~(kWave - 1)); u0 < units; u0 += stride) {
        const int64_t u = u0 + (threadIdx.x & (kWave - 1));
        const bool in = u < units;
        if (VEC) {
            float4 fv = {0.0f, 0.0f, 0.0f, 0.0f}, mv = fv;
            uint32_t k = 0;
            if (in) {
                fv = reinterpret_cast<const float4*>(f)[u];
                mv = reinterpret_cast<const float4*>(m)[u];
                k = mask ? reinterpret_cast<const uint32_t*>(mask)[u] : 0x01010101u;
            }
            const float fa[4] = {fv.x, fv.y, fv.z, fv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const SimVoxel vx = sim_voxel(fa[s], ma[s], ((k >> (8 * s)) & 0xFFu) != 0, bn, a);
                hist_add(h, vx.take, vx.cell, aggregate);
            }
        } else {
            float fs = 0.0f, ms = 0.0f;
            bool k = false;
            if (in) {
                fs = f[u];
                ms = m[u];
                k = mask ? mask[u] != 0 : true;
            }
            const SimVoxel vx = sim_voxel(fs, ms, k, bn, a);
            hist_add(h, vx.take, vx.cell, aggregate);
        }
    }
    __syncthreads();
    int32_t* hc = hist + (int64_t)chain * cells;
    for (int i = threadIdx.x; i < cells; i += kBlock) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&hc[i], (int32_t)c);
    }
    __syncthreads();  // the histogram has left: its first bytes serve the block reduction
    sim_block_reduce(a, reinterpret_cast<double*>(sim_lds));
    if (threadIdx.x == 0) a.store(ipart, fpart, (int64_t)chain * gridDim.x + blockIdx.x);
}

// -p ln p of a count c out of n (0 for an empty cell)
__device__ __forceinline__ double entropy_term(long long c, double n) {
    if (c <= 0) return 0.0;
    const double p = (double)c / n;
    return -p * log(p);
}

// one block of kFinishBlock threads per chain: hist (C,B,B), the chain's `nblocks` rows of partials -> stats (C,
// IRS_SIMILARITY_STATS).  Sixteen wavefronts, not four: the double-precision log of a cell is about half a microsecond for a
// wavefront alone on its SIMD, and the cells of a thread come one after the other.
constexpr int kFinishBlock = 1024;
static_assert(kSimMaxBlocks <= kFinishBlock, "the finish kernel folds one row of partials per thread");

__global__ __launch_bounds__(kFinishBlock) void similarity_finish_kernel(const int32_t* __restrict__ hist, int B,
                                                                         const long long* __restrict__ ipart,
                                                                         const double* __restrict__ fpart, int nblocks,
                                                                         double* __restrict__ stats) {
    constexpr int G = kFinishBlock / kWave;
    constexpr int kMaxCells = IRS_SIMILARITY_MAX_BINS * IRS_SIMILARITY_MAX_BINS;
    __shared__ int32_t hl[kMaxCells];  // the chain's histogram: 64 KB of gfx950's 160
    __shared__ double acc_smem[kSimCols * G];
    __shared__ double hsmem[3 * G];
    __shared__ long long n_shared;
    const int chain = blockIdx.x;
    const int cells = B * B;

    // Every load first, then the arithmetic: the cells were written by atomics, which leave nothing in L2, and the partial
    // rows by other CUs -- a load per loop trip would pay that latency once per trip.  The loops below stay rolled.
    constexpr int kLoads = kMaxCells / kFinishBlock;
    const int32_t* hc = hist + (int64_t)chain * cells;
    int32_t cell[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int i = threadIdx.x + k * kFinishBlock;
        cell[k] = i < cells ? hc[i] : 0;
    }
    // thread i takes row i of the partials: lanes by the shuffle butterfly, then the wavefronts in order
    SimAcc a = (int)threadIdx.x < nblocks ? SimAcc::load(ipart, fpart, (int64_t)chain * nblocks + threadIdx.x) : SimAcc::identity();
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int i = threadIdx.x + k * kFinishBlock;
        if (i < cells) hl[i] = cell[k];
    }
    sim_block_reduce<G>(a, acc_smem);
    if (threadIdx.x == 0) n_shared = a.i[0];
    __syncthreads();  // hl and n_shared
    const double n = (double)n_shared;

    // joint entropy: thread i takes cells i, i + 1024, ...; threads 0 .. B - 1 a column each, threads 128 .. 128 + B - 1 a row
    // each, walked from its own diagonal so that the lanes of a wavefront stay on different LDS banks
    double hj = 0.0, hf = 0.0, hm = 0.0;
#pragma unroll 1
    for (int i = threadIdx.x; i < cells; i += kFinishBlock) hj += entropy_term(hl[i], n);
    const int t = threadIdx.x & (IRS_SIMILARITY_MAX_BINS - 1);
    if (threadIdx.x < 2 * IRS_SIMILARITY_MAX_BINS && t < B) {
        const bool rows = threadIdx.x >= IRS_SIMILARITY_MAX_BINS;
        long long c = 0;
#pragma unroll 1
        for (int k = 0; k < B; ++k) {
            const int j = t + k < B ? t + k : t + k - B;
            c += rows ? hl[t * B + j] : hl[k * B + t];
        }
        (rows ? hf : hm) = entropy_term(c, n);
    }
    double hv[3] = {hf, hm, hj};
    block_sum<3, G>(hv, hsmem);

    if (threadIdx.x == 0) {
        double* s = stats + (int64_t)chain * IRS_SIMILARITY_STATS;
        const double nan = __builtin_nan("");
        s[0] = n;
        s[1] = (double)a.i[1];
        s[2] = (double)a.i[2];
        const bool any = a.i[0] > 0;
        const double mf = a.f[1] / n, mm = a.f[2] / n;
        const double var_f = a.f[3] / n - mf * mf, var_m = a.f[4] / n - mm * mm;
        s[3] = any ? a.f[0] / n : nan;
        s[4] = any && var_f > 0.0 && var_m > 0.0 ? (a.f[5] / n - mf * mm) / sqrt(var_f * var_m) : nan;
        s[5] = any ? hv[0] : nan;
        s[6] = any ? hv[1] : nan;
        s[7] = any ? hv[2] : nan;
        s[8] = any ? hv[0] + hv[1] - hv[2] : nan;
        s[9] = any && hv[2] != 0.0 ? (hv[0] + hv[1]) / hv[2] : nan;
    }
}

}  // namespace

// blocks per chain: the grid depends on (V, C) only
static int similarity_blocks(int64_t V, int C, bool vec) {
    const int64_t units = vec ? V >> 2 : V;
    return (int)std::max<int64_t>(1, std::min<int64_t>((units + kBlock - 1) / kBlock, kSimMaxBlocks / C));
}

void launch_image_similarity(const float* fixed, int64_t fixed_stride, const float* moving, const uint8_t* mask, int64_t V, int C,
                             const SimBins& bn, int32_t* hist, double* stats, long long* ipart, double* fpart, hipStream_t st) {
    const bool vec = (V & 3) == 0 && (((uintptr_t)fixed | (uintptr_t)moving) & 15) == 0 && ((uintptr_t)mask & 3) == 0;
    const int blocks = similarity_blocks(V, C, vec);
    const bool aggregate = global_knobs().similarity_aggregate != 0;
    const size_t lds = std::max<size_t>((size_t)bn.bins * bn.bins * sizeof(uint32_t), sizeof(double) * kSimCols * (kBlock / kWave));
    (void)hipMemsetAsync(hist, 0, (size_t)C * bn.bins * bn.bins * sizeof(int32_t), st);
    if (vec)
        hipLaunchKernelGGL(similarity_accumulate_kernel<true>, dim3(blocks, C), dim3(kBlock), lds, st, fixed, fixed_stride, moving,
                           mask, V, bn, aggregate, hist, ipart, fpart);
    else
        hipLaunchKernelGGL(similarity_accumulate_kernel<false>, dim3(blocks, C), dim3(kBlock), lds, st, fixed, fixed_stride, moving,
                           mask, V, bn, aggregate, hist, ipart, fpart);
    hipLaunchKernelGGL(similarity_finish_kernel, dim3(C), dim3(kFinishBlock), 0, st, hist, bn.bins, ipart, fpart, blocks, stats);
}

}  // namespace irs
