// The mutual-information data term (absent in the reference, whose data losses compare intensities voxel by voxel; DESIGN.md
// section 6; the definition: include/irsgmcmc.h, irs_mi_fwd): a Mattes-style Parzen joint histogram of the fixed and the (warped)
// moving image -- zero-order window on the fixed intensity, cubic B-spline window on the moving one -- in Q30 fixed point, the
// table T = ln(p_ab / (p_a p_b)) and MI = sum p_ab T from it, and the gradient of MI with respect to the moving image.
//
//  - accumulate: one launch for all chains, blockIdx.y the chain: the grid-stride stream of similarity_accumulate_kernel (9 bytes per
//    voxel and chain; four voxels per 16-byte load when V % 4 == 0 and the bases are aligned).  A voxel takes part when its mask is
//    set (or absent) and both intensities are finite; it adds q_0 .. q_3 with q_0 + .. + q_3 = 2^30 exactly to the cells (a, k0 - 1
//    .. k0 + 2) of the block's B x B uint64 histogram in LDS (8 KB at 32 bins, 32 KB at 64): four 64-bit LDS atomics, always (wave
//    aggregation measured slower: mi_add).  At the end the
//    non-zero cells go to the chain's global uint64 histogram with integer atomics -- exact, so their order does not matter -- and
//    the three counts to one row of partials per block (SummaryAcc).
//  - finish: one block of 512 threads per chain stages the histogram in LDS, folds the rows of counts, forms the integer row and
//    column sums without atomics and writes T (float32), the entropies, MI, n and the data term, every sum a double in a fixed
//    order.  The global histogram stays as it is (a caller may read it): the forward launcher zeroes it with a stream-ordered memset
//    in front of the accumulate kernel.
//  - gradient: the stream again, with the chain's T in LDS (B * B floats): it recomputes a, k0 and u with the device function the
//    accumulate kernel used, makes four LDS reads and writes g and, when asked, the pmi map.  9 bytes in, 4 .. 8 out, no atomics.
// Integer histogram, fixed-order double sums, nothing that depends on the launch shape: two calls give the same bits, and chain c of
// a batch is the single-chain call.
#include <algorithm>

#include "kernels.h"
#include "mi_device.h"
#include "summary_device.h"

namespace irs {
namespace {

// integer sums {voxels taking part, masked voxels with a non-finite intensity, taking voxels with a clipped intensity}
struct MiSummary {
    static constexpr int kInts = 3, kFloats = 0;
    static constexpr Col kind(int) { return Col::Sum; }
};
using MiAcc = SummaryAcc<MiSummary>;

constexpr int kMiMaxBlocks = IRS_MI_MAX_BLOCKS;  // all chains together
constexpr int kMiMaxCells = IRS_MI_MAX_BINS * IRS_MI_MAX_BINS;
typedef unsigned long long u64;

// the four taps of one voxel into the block's histogram: four LDS atomics.  Wave aggregation -- a wavefront whose taking lanes all
// share (a, k0) adding one wave-reduced q_j per tap, the idea of hist_add's `aggregate` -- was built and measured, and lost on the
// synthetic pair AND on a constant image (256^3: 76.1 against 72.1 us; the whole forward call on a constant image 132.6 against 128.8
// us): its three 64-bit butterflies cost more than the serialised adds they replace.
__device__ __forceinline__ void mi_add(u64* h, const MiVoxel& v, int bins) {
    if (!v.take) return;
    double w[4];
    u64 q[4];
    mi_weights(v.m.u, w);
    mi_fixed_point(w, q);
    const int cell = v.a * bins + v.m.k0 - 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) atomicAdd(&h[cell + j], q[j]);
}

__device__ __forceinline__ void mi_count(const MiVoxel& v, float f, bool masked, const MiBins& bn, MiAcc& a) {
    a.i[0] += v.take;
    a.i[1] += masked && !v.take;
    a.i[2] += v.take && (f < bn.f_lo || f > bn.f_hi || !v.m.inside);
}

// fixed (1 or C,V) with fixed_stride 0 or V; moving (C,V); mask (1 or C,V) with mask_stride 0 or V, or nullptr; hist (C,B,B), zero
// on entry; row blockIdx.x of the chain's partials.  VEC: V % 4 == 0, fixed / moving 16-byte and mask 4-byte aligned.  Dynamic
// LDS: B * B * 8 bytes (at least sizeof(MiAcc) * kBlock / kWave).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void mi_accumulate_kernel(const float* __restrict__ fixed, int64_t fixed_stride,
                                                               const float* __restrict__ moving, const uint8_t* __restrict__ mask,
                                                               int64_t mask_stride, int64_t V, MiBins bn,
                                                               u64* __restrict__ hist, long long* __restrict__ ipart) {
    extern __shared__ __align__(16) unsigned char mi_lds[];
    u64* h = reinterpret_cast<u64*>(mi_lds);
    const int cells = bn.bins * bn.bins;
    for (int i = threadIdx.x; i < cells; i += kBlock) h[i] = 0;
    __syncthreads();

    const int chain = blockIdx.y;
    const float* f = fixed + (int64_t)chain * fixed_stride;
    const float* m = moving + (int64_t)chain * V;
    const uint8_t* k = mask ? mask + (int64_t)chain * mask_stride : nullptr;
    MiAcc a = MiAcc::identity();
    const int64_t units = VEC ? V >> 2 : V;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < units; u += stride) {
        if (VEC) {
            const float4 fv = reinterpret_cast<const float4*>(f)[u], mv = reinterpret_cast<const float4*>(m)[u];
            const uint32_t kv = k ? reinterpret_cast<const uint32_t*>(k)[u] : 0x01010101u;
            const float fa[4] = {fv.x, fv.y, fv.z, fv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bool masked = ((kv >> (8 * s)) & 0xFFu) != 0;
                const MiVoxel vx = mi_voxel(fa[s], ma[s], masked, bn);
                mi_count(vx, fa[s], masked, bn, a);
                mi_add(h, vx, bn.bins);
            }
        } else {
            const float fs = f[u], ms = m[u];
            const bool masked = k ? k[u] != 0 : true;
            const MiVoxel vx = mi_voxel(fs, ms, masked, bn);
            mi_count(vx, fs, masked, bn, a);
            mi_add(h, vx, bn.bins);
        }
    }
    __syncthreads();
    u64* hc = hist + (int64_t)chain * cells;
    for (int i = threadIdx.x; i < cells; i += kBlock) {
        const u64 c = h[i];
        if (c) atomicAdd(&hc[i], c);
    }
    __syncthreads();  // the histogram has left: its first bytes serve the block reduction
    a.block_reduce(reinterpret_cast<MiAcc*>(mi_lds));
    if (threadIdx.x == 0) a.store(ipart, nullptr, (int64_t)chain * gridDim.x + blockIdx.x);
}

constexpr int kMiFinishBlock = 512;  // (1024 threads leave 128 VGPRs each: the double-precision log would spill)
static_assert(kMiMaxCells % kMiFinishBlock == 0, "the finish kernel loads kMiMaxCells / kMiFinishBlock cells per thread");

// one block per chain: hist (C,B,B) and the chain's `nblocks` rows of counts -> table (C,B,B) float32, stats (C, IRS_MI_STATS) and,
// when given, data_out[chain * data_stride] = weight * n * (ln B - MI)
__global__ __launch_bounds__(kMiFinishBlock) void mi_finish_kernel(const u64* __restrict__ hist, int B,
                                                                   const long long* __restrict__ ipart, int nblocks,
                                                                   float* __restrict__ table, double* __restrict__ stats, double weight,
                                                                   double* __restrict__ data_out, int64_t data_stride) {
    constexpr int G = kMiFinishBlock / kWave;
    __shared__ u64 hl[kMiMaxCells];  // 32 KB
    __shared__ u64 rows[IRS_MI_MAX_BINS], cols[IRS_MI_MAX_BINS];
    __shared__ double smem[5 * G];
    const int chain = blockIdx.x;
    const int cells = B * B;

    // every load first (the cells were written by atomics of other CUs), then the arithmetic
    constexpr int kLoads = kMiMaxCells / kMiFinishBlock;
    const u64* hc = hist + (int64_t)chain * cells;
    u64 cell[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int i = threadIdx.x + k * kMiFinishBlock;
        cell[k] = i < cells ? hc[i] : 0;
    }
    long long bad = 0, clipped = 0;  // thread i takes rows i, i + 512 of the counts (n itself comes from the histogram)
    for (int r = threadIdx.x; r < nblocks; r += kMiFinishBlock) {
        const long long* row = ipart + ((int64_t)chain * nblocks + r) * MiSummary::kInts;
        bad += row[1];
        clipped += row[2];
    }
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int i = threadIdx.x + k * kMiFinishBlock;
        if (i < cells) hl[i] = cell[k];
    }
    __syncthreads();
    // threads 0 .. B - 1 a column each, threads 64 .. 64 + B - 1 a row each, walked from its own diagonal so that the lanes of a
    // wavefront stay on different LDS banks.  Integer sums: the order does not matter.
    const int t = threadIdx.x & (IRS_MI_MAX_BINS - 1);
    if (threadIdx.x < 2 * IRS_MI_MAX_BINS && t < B) {
        const bool is_row = threadIdx.x >= IRS_MI_MAX_BINS;
        u64 c = 0;
#pragma unroll 1
        for (int k = 0; k < B; ++k) {
            const int j = t + k < B ? t + k : t + k - B;
            c += is_row ? hl[t * B + j] : hl[j * B + t];
        }
        (is_row ? rows : cols)[t] = c;
    }
    __syncthreads();
    u64 total = 0;  // n 2^30
#pragma unroll 1
    for (int k = 0; k < B; ++k) total += rows[k];
    const double N = (double)total;

    // T_ab = ln(p_ab / (p_a p_b)), 0 in an empty cell; thread i takes cells i, i + 512, ...
    double mi = 0.0, hf = 0.0, hm = 0.0;
    float* tc = table + (int64_t)chain * cells;
#pragma unroll 1
    for (int i = threadIdx.x; i < cells; i += kMiFinishBlock) {
        const u64 c = hl[i];
        double T = 0.0;
        if (c) {
            const double p = (double)c / N, pa = (double)rows[i / B] / N, pb = (double)cols[i % B] / N;
            T = log(p / (pa * pb));
            mi += p * T;
        }
        tc[i] = (float)T;
    }
    if (threadIdx.x < 2 * IRS_MI_MAX_BINS && t < B) {
        const u64 c = threadIdx.x >= IRS_MI_MAX_BINS ? rows[t] : cols[t];
        if (c) {
            const double p = (double)c / N;
            (threadIdx.x >= IRS_MI_MAX_BINS ? hf : hm) = -p * log(p);
        }
    }
    double v[5] = {mi, hf, hm, (double)bad, (double)clipped};  // (the counts: below 2^30, exact as doubles)
    block_sum<5, G>(v, smem);
    if (threadIdx.x == 0) {
        const double n = (double)(total >> kMiQ);
        const double term = total ? n * (log((double)B) - v[0]) : 0.0;
        double* s = stats + (int64_t)chain * IRS_MI_STATS;
        s[0] = n;
        s[1] = v[3];
        s[2] = v[4];
        s[3] = v[0];
        s[4] = v[1];
        s[5] = v[2];
        s[6] = term;
        if (data_out) data_out[(int64_t)chain * data_stride] = weight * term;
    }
}

struct MiOut {
    float g, pmi;
};

// one voxel of the gradient: T the chain's table in LDS; coef = -weight * scale * (B - 3) / (m_hi - m_lo) of the chain
__device__ __forceinline__ MiOut mi_gradient(float f, float m, bool masked, const MiBins& bn, const float* T, double coef, double lnB,
                                             bool residual_form) {
    const MiVoxel v = mi_voxel(f, m, masked, bn);
    MiOut o = {0.0f, 0.0f};
    if (!v.take) return o;
    const float* row = T + v.a * bn.bins + v.m.k0 - 1;
    const double t0 = (double)row[0], t1 = (double)row[1], t2 = (double)row[2], t3 = (double)row[3];
    double w[4], d[4];
    mi_weights(v.m.u, w);
    mi_weight_derivatives(v.m.u, d);
    const double pmi = __dadd_rn(__dadd_rn(__dmul_rn(w[0], t0), __dmul_rn(w[1], t1)), __dadd_rn(__dmul_rn(w[2], t2), __dmul_rn(w[3], t3)));
    const double s = __dadd_rn(__dadd_rn(__dmul_rn(d[0], t0), __dmul_rn(d[1], t1)), __dadd_rn(__dmul_rn(d[2], t2), __dmul_rn(d[3], t3)));
    o.pmi = (float)(residual_form ? lnB - pmi : pmi);
    o.g = v.m.inside ? (float)__dmul_rn(coef, s) : 0.0f;
    return o;
}

// table (C,B,B) of mi_finish_kernel; scale: C floats on the device or nullptr (1); g (C,V), pmi (C,V) or nullptr.  residual_form:
// pmi receives ln B - pmi at the voxels that take part (0 elsewhere in both forms).  Dynamic LDS: B * B floats.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void mi_gradient_kernel(const float* __restrict__ fixed, int64_t fixed_stride,
                                                             const float* __restrict__ moving, const uint8_t* __restrict__ mask,
                                                             int64_t mask_stride, const float* __restrict__ table, int64_t V, MiBins bn,
                                                             float weight, const float* __restrict__ scale, bool residual_form,
                                                             float* __restrict__ g, float* __restrict__ pmi) {
    extern __shared__ __align__(16) unsigned char mi_lds[];
    float* T = reinterpret_cast<float*>(mi_lds);
    const int chain = blockIdx.y;
    const int cells = bn.bins * bn.bins;
    for (int i = threadIdx.x; i < cells; i += kBlock) T[i] = table[(int64_t)chain * cells + i];
    __syncthreads();

    const float* f = fixed + (int64_t)chain * fixed_stride;
    const float* m = moving + (int64_t)chain * V;
    const uint8_t* k = mask ? mask + (int64_t)chain * mask_stride : nullptr;
    float* gc = g + (int64_t)chain * V;
    float* pc = pmi ? pmi + (int64_t)chain * V : nullptr;
    const double coef = -__dmul_rn(__dmul_rn((double)weight, scale ? (double)scale[chain] : 1.0), bn.m_scale);
    const double lnB = log((double)bn.bins);
    const int64_t units = VEC ? V >> 2 : V;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < units; u += stride) {
        if (VEC) {
            const float4 fv = reinterpret_cast<const float4*>(f)[u], mv = reinterpret_cast<const float4*>(m)[u];
            const uint32_t kv = k ? reinterpret_cast<const uint32_t*>(k)[u] : 0x01010101u;
            const float fa[4] = {fv.x, fv.y, fv.z, fv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w};
            MiOut o[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) o[s] = mi_gradient(fa[s], ma[s], ((kv >> (8 * s)) & 0xFFu) != 0, bn, T, coef, lnB, residual_form);
            reinterpret_cast<float4*>(gc)[u] = make_float4(o[0].g, o[1].g, o[2].g, o[3].g);
            if (pc) reinterpret_cast<float4*>(pc)[u] = make_float4(o[0].pmi, o[1].pmi, o[2].pmi, o[3].pmi);
        } else {
            const MiOut o = mi_gradient(f[u], m[u], k ? k[u] != 0 : true, bn, T, coef, lnB, residual_form);
            gc[u] = o.g;
            if (pc) pc[u] = o.pmi;
        }
    }
}

bool mi_vec(int64_t V, const void* a, const void* b, const void* c, const void* d, const uint8_t* mask) {
    return (V & 3) == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0 && ((uintptr_t)mask & 3) == 0;
}

}  // namespace

// blocks per chain: the grid depends on (V, C) and the form only
int mi_blocks(int64_t V, int C, bool vec) {
    const int64_t units = vec ? V >> 2 : V;
    return (int)std::max<int64_t>(1, std::min<int64_t>((units + kBlock - 1) / kBlock, kMiMaxBlocks / C));
}

hipError_t launch_mi_fwd(const float* fixed, int64_t fixed_stride, const float* moving, const uint8_t* mask, int64_t mask_stride, int64_t V,
                   int C, const MiBins& bn, unsigned long long* hist, float* table, double* stats, long long* ipart, double weight,
                   double* data_out, int64_t data_stride, hipStream_t st) {
    const bool vec = mi_vec(V, fixed, moving, nullptr, nullptr, mask);
    const int blocks = mi_blocks(V, C, vec);
    const size_t cells = (size_t)bn.bins * bn.bins;
    const size_t lds = std::max<size_t>(cells * sizeof(u64), sizeof(MiAcc) * (kBlock / kWave));
    // (a memset that failed would leave the accumulate kernel adding to a stale histogram: the caller gets its status)
    const hipError_t cleared = hipMemsetAsync(hist, 0, (size_t)C * cells * sizeof(u64), st);
    if (cleared != hipSuccess) return cleared;
    if (vec)
        hipLaunchKernelGGL(mi_accumulate_kernel<true>, dim3(blocks, C), dim3(kBlock), lds, st, fixed, fixed_stride, moving, mask,
                           mask_stride, V, bn, hist, ipart);
    else
        hipLaunchKernelGGL(mi_accumulate_kernel<false>, dim3(blocks, C), dim3(kBlock), lds, st, fixed, fixed_stride, moving, mask,
                           mask_stride, V, bn, hist, ipart);
    hipLaunchKernelGGL(mi_finish_kernel, dim3(C), dim3(kMiFinishBlock), 0, st, hist, bn.bins, ipart, blocks, table, stats, weight,
                       data_out, data_stride);
    return hipSuccess;
}

void launch_mi_bwd(const float* fixed, int64_t fixed_stride, const float* moving, const uint8_t* mask, int64_t mask_stride,
                   const float* table, int64_t V, int C, const MiBins& bn, float weight, const float* scale, bool residual_form,
                   float* g, float* pmi, hipStream_t st) {
    const bool vec = mi_vec(V, fixed, moving, g, pmi, mask);
    const int blocks = mi_blocks(V, C, vec);
    const size_t lds = (size_t)bn.bins * bn.bins * sizeof(float);
    if (vec)
        hipLaunchKernelGGL(mi_gradient_kernel<true>, dim3(blocks, C), dim3(kBlock), lds, st, fixed, fixed_stride, moving, mask,
                           mask_stride, table, V, bn, weight, scale, residual_form, g, pmi);
    else
        hipLaunchKernelGGL(mi_gradient_kernel<false>, dim3(blocks, C), dim3(kBlock), lds, st, fixed, fixed_stride, moving, mask,
                           mask_stride, table, V, bn, weight, scale, residual_form, g, pmi);
}

}  // namespace irs
