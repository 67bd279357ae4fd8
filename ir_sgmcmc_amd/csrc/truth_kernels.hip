// Known-transformation validation (absent in the reference): the recorded displacement against a dense truth, and the
// calibration of the displacement covariance posterior against it ("Known-transformation validation"; the
// arithmetic is truth_device.h).
//
//  - update: one grid-stride stream over the voxels for all C chains, C a template parameter so that the per-chain accumulators
//    stay in registers.  A thread reads the truth and its three rank counts once, then every chain's sample: 12 C + 12 + 6 + 6
//    (+ 1 with a mask) bytes per voxel.  The counts are the thread's own voxel: plain read-modify-writes.  The per-chain sums
//    are reduced over the block by summary_device.h and stored as one row of partials per (chain, block);
//    truth_rows_reduce_kernel, one block per chain, folds them in block order.
//  - calibrate: one grid-stride stream, one voxel per thread and round: 50 bytes in, 8 out.  The integer tables are counted in
//    LDS (uint32: a block sees at most 2^20 voxels) and added to the int64 outputs by integer atomics, which are exact in any
//    order; the double sums of the reliability table go through the labelled reduction of structure_device.h with the bin as
//    the label, the summary through summary_device.h.
// The grids depend on the volume alone and every floating-point merge has a fixed place: two identical calls are bit-identical.
#include <algorithm>

#include "kernels.h"
#include "structure_device.h"
#include "truth_device.h"

namespace irs {
namespace {

using UpdateAcc = SummaryAcc<TruthUpdate>;
using CalAcc = SummaryAcc<TruthSummary>;
using RelAcc = SummaryAcc<TruthReliability>;

constexpr int kUpdateChunk = IRS_TRUTH_UPDATE_WS_BYTES / IRS_MAX_CHAINS;  // bytes of partials of one chain
constexpr int kCalibrateBlocks = 1024;

struct Scale3d {
    double s[3];
};

// u (C,3,V), t (3,V) float32; below (3,V) uint16; mask (V) uint8 or nullptr; partials of chain c at ws + c * kUpdateChunk
template <int C>
__global__ __launch_bounds__(kBlock) void truth_update_kernel(const float* __restrict__ u, const float* __restrict__ t,
                                                              uint16_t* __restrict__ below, const uint8_t* __restrict__ mask,
                                                              Scale3d scale, int records_before, int64_t V, char* __restrict__ ws,
                                                              int nblocks) {
    __shared__ UpdateAcc smem[UpdateAcc::kG];
    UpdateAcc acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = UpdateAcc::identity();
    const double s[3] = {scale.s[0], scale.s[1], scale.s[2]};
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        float tv[3];
        unsigned cnt[3] = {0u, 0u, 0u};
#pragma unroll
        for (int a = 0; a < 3; ++a) tv[a] = t[a * V + v];
        if (records_before > 0) {  // the first record of all overwrites: a fresh state is never read
#pragma unroll
            for (int a = 0; a < 3; ++a) cnt[a] = below[a * V + v];
        }
        const bool in = !mask || mask[v];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float uv[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                uv[a] = u[((int64_t)c * 3 + a) * V + v];
                cnt[a] += uv[a] < tv[a] ? 1u : 0u;
            }
            if (in) truth_error_fold(uv, tv, s, acc[c]);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) below[a * V + v] = (uint16_t)cnt[a];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c > 0) __syncthreads();  // smem is read by thread 0 of the reduction before
        acc[c].block_reduce(smem);
        if (threadIdx.x == 0) {
            long long* ip = (long long*)(ws + (size_t)c * kUpdateChunk);
            acc[c].store(ip, (double*)(ip + (size_t)TruthUpdate::kInts * nblocks), blockIdx.x);
        }
    }
}

// one block per chain: its nblocks rows of partials folded as summary_reduce_kernel folds them -> row `chain` of ints / floats
__global__ __launch_bounds__(kBlock) void truth_rows_reduce_kernel(const char* __restrict__ ws, int nblocks, long long* __restrict__ ints,
                                                                   double* __restrict__ floats) {
    __shared__ UpdateAcc smem[UpdateAcc::kG];
    const long long* ip = (const long long*)(ws + (size_t)blockIdx.x * kUpdateChunk);
    const double* fp = (const double*)(ip + (size_t)TruthUpdate::kInts * nblocks);
    UpdateAcc a = UpdateAcc::identity();
    for (int b = threadIdx.x; b < nblocks; b += kBlock) a.merge(UpdateAcc::load(ip, fp, b));
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ints, floats, blockIdx.x);
}

struct CalibrateTables {
    double d2_edges[IRS_TRUTH_MAX_BINS - 1];
    double levels[IRS_TRUTH_MAX_LEVELS];
    double var_edges[IRS_TRUTH_MAX_RELIABILITY_BINS - 1];
    int B, L, Br, R;
};

constexpr int kMaxCounts = IRS_TRUTH_COUNTS(IRS_TRUTH_MAX_BINS, IRS_TRUTH_MAX_LEVELS, IRS_TRUTH_MAX_BINS);

// mean (3,V), comoment (6,V), truth (3,V) float32, below (3,V) uint16 after n records -> error, mahalanobis (V) float32, the
// integer tables (added to `counts`, zeroed before the launch), and per block the partials of the reliability table and of the
// summary
__global__ __launch_bounds__(kBlock) void truth_calibrate_kernel(const float* __restrict__ mean, const float* __restrict__ comoment,
                                                                 const uint16_t* __restrict__ below, const float* __restrict__ truth,
                                                                 int64_t V, int n, Scale3d scale, double f2,
                                                                 const uint8_t* __restrict__ mask, CalibrateTables tb,
                                                                 float* __restrict__ error, float* __restrict__ mahalanobis,
                                                                 unsigned long long* __restrict__ counts, long long* __restrict__ rel_ipart,
                                                                 double* __restrict__ rel_fpart, long long* __restrict__ ipart,
                                                                 double* __restrict__ fpart) {
    __shared__ CalAcc smem[CalAcc::kG];
    __shared__ StructureTables<TruthReliability> rel;
    __shared__ uint32_t hist[kMaxCounts];
    const int ncounts = IRS_TRUTH_COUNTS(tb.B, tb.L, tb.Br);
    for (int e = threadIdx.x; e < ncounts; e += kBlock) hist[e] = 0u;
    rel.clear(tb.R);  // ends in a barrier
    CalAcc a = CalAcc::identity();
    const double s[3] = {scale.s[0], scale.s[1], scale.s[2]};
    const double nm1 = (double)(n - 1);
    const float nanf_ = __builtin_nanf("");
    // `base` is uniform over the block: every lane of a wavefront reaches the labelled fold of every round
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < V; base += (int64_t)gridDim.x * kBlock) {
        const int64_t v = base + threadIdx.x;
        int bin = -1;
        RelAcc ra = RelAcc::identity();
        if (v < V) {
            float mu[3], M[6], t[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) mu[c] = mean[c * V + v], t[c] = truth[c * V + v];
#pragma unroll
            for (int c = 0; c < 6; ++c) M[c] = comoment[c * V + v];
            const TruthVoxel o = truth_calibrate_voxel(mu, M, t, s, nm1, f2);
            const double err = __dsqrt_rn(o.err2);
            error[v] = o.finite ? (float)err : nanf_;
            mahalanobis[v] = o.finite ? (float)__dsqrt_rn(o.dist2) : nanf_;
            if (!mask || mask[v]) {
                a.i[0] += 1;
                if (o.finite) {
                    a.i[2] += o.raised ? 1 : 0;
                    a.f[0] += err;
                    a.f[1] += o.err2;
                    a.f[2] = fmax(a.f[2], err);
                    a.f[3] += o.dist2;
                    a.f[4] = fmax(a.f[4], o.dist2);
                    a.f[5] += o.v;
                    a.f[6] += o.z[0];
                    a.f[7] += o.z[1];
                    a.f[8] += o.z[2];
                    atomicAdd(&hist[truth_bin(tb.d2_edges, tb.B - 1, o.dist2)], 1u);
                    for (int l = 0; l < tb.L; ++l)
                        if (o.dist2 <= tb.levels[l]) atomicAdd(&hist[tb.B + l], 1u);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int rb = min((int)below[c * V + v] * tb.Br / (n + 1), tb.Br - 1);
                        atomicAdd(&hist[tb.B + tb.L + c * tb.Br + rb], 1u);
                    }
                    bin = min(truth_bin(tb.var_edges, tb.R - 1, o.v), tb.R - 1);  // (a NaN v is <= no edge: bin 0)
                    ra.i[0] = 1;
                    ra.f[0] = o.v;
                    ra.f[1] = o.err2;
                } else {
                    a.i[1] += 1;
                }
            }
        }
        structure_wave_fold(bin, ra, rel);
    }
    structure_block_store(rel, tb.R, 0, rel_ipart, rel_fpart);  // begins with a barrier: the LDS counts are complete, too
    for (int e = threadIdx.x; e < ncounts; e += kBlock)
        if (hist[e]) atomicAdd(&counts[e], (unsigned long long)hist[e]);
    a.block_reduce(smem);
    if (threadIdx.x == 0) a.store(ipart, fpart, blockIdx.x);
}

template <int C>
void launch_update_c(const float* u, const float* t, uint16_t* below, const uint8_t* mask, const Scale3d& sc, int records_before,
                     int64_t V, char* ws, int blocks, hipStream_t st) {
    hipLaunchKernelGGL(truth_update_kernel<C>, dim3(blocks), dim3(kBlock), 0, st, u, t, below, mask, sc, records_before, V, ws, blocks);
}

}  // namespace

void launch_truth_update(const float* displacement, int C, const float* truth, uint16_t* below, const uint8_t* mask, const float* scale,
                         int records_before, int64_t V, long long* ints, double* floats, void* ws, hipStream_t st) {
    // every chain has the same share of the workspace whatever C is: the grid depends on the volume only
    const int blocks = (int)std::min<int64_t>((V + kBlock - 1) / kBlock, kUpdateChunk / (TruthUpdate::kInts + TruthUpdate::kFloats) / 8);
    const Scale3d sc{{(double)scale[0], (double)scale[1], (double)scale[2]}};
    char* w = (char*)ws;
    switch (C) {
        case 1: launch_update_c<1>(displacement, truth, below, mask, sc, records_before, V, w, blocks, st); break;
        case 2: launch_update_c<2>(displacement, truth, below, mask, sc, records_before, V, w, blocks, st); break;
        case 3: launch_update_c<3>(displacement, truth, below, mask, sc, records_before, V, w, blocks, st); break;
        case 4: launch_update_c<4>(displacement, truth, below, mask, sc, records_before, V, w, blocks, st); break;
        case 5: launch_update_c<5>(displacement, truth, below, mask, sc, records_before, V, w, blocks, st); break;
        case 6: launch_update_c<6>(displacement, truth, below, mask, sc, records_before, V, w, blocks, st); break;
        case 7: launch_update_c<7>(displacement, truth, below, mask, sc, records_before, V, w, blocks, st); break;
        default: launch_update_c<8>(displacement, truth, below, mask, sc, records_before, V, w, blocks, st); break;
    }
    static_assert(IRS_MAX_CHAINS == 8, "one instantiation per chain count");
    hipLaunchKernelGGL(truth_rows_reduce_kernel, dim3(C), dim3(kBlock), 0, st, (const char*)w, blocks, ints, floats);
}

void launch_truth_calibrate(const float* mean, const float* comoment, const uint16_t* below, const float* truth, int64_t V, int n,
                            const float* scale, double std_floor, const uint8_t* mask, const double* d2_edges, int B,
                            const double* levels, int L, int Br, const double* var_edges, int R, float* error, float* mahalanobis,
                            long long* counts, long long* rel_ints, double* rel_floats, long long* isummary, double* fsummary,
                            void* ws, hipStream_t st) {
    const int blocks = (int)std::min<int64_t>((V + kBlock - 1) / kBlock, kCalibrateBlocks);
    // the workspace: the summary's partials, then the reliability table's [bin][block][column]
    long long* ipart = (long long*)ws;
    double* fpart = (double*)(ipart + (size_t)TruthSummary::kInts * blocks);
    long long* rel_ipart = (long long*)(fpart + (size_t)TruthSummary::kFloats * blocks);
    double* rel_fpart = (double*)(rel_ipart + (size_t)R * blocks * TruthReliability::kInts);
    CalibrateTables tb;
    for (int e = 0; e < IRS_TRUTH_MAX_BINS - 1; ++e) tb.d2_edges[e] = e < B - 1 ? d2_edges[e] : 0.0;
    for (int e = 0; e < IRS_TRUTH_MAX_LEVELS; ++e) tb.levels[e] = e < L ? levels[e] : 0.0;
    for (int e = 0; e < IRS_TRUTH_MAX_RELIABILITY_BINS - 1; ++e) tb.var_edges[e] = e < R - 1 ? var_edges[e] : 0.0;
    tb.B = B, tb.L = L, tb.Br = Br, tb.R = R;
    const Scale3d sc{{(double)scale[0], (double)scale[1], (double)scale[2]}};
    (void)hipMemsetAsync(counts, 0, sizeof(long long) * IRS_TRUTH_COUNTS(B, L, Br), st);
    hipLaunchKernelGGL(truth_calibrate_kernel, dim3(blocks), dim3(kBlock), 0, st, mean, comoment, below, truth, V, n, sc,
                       std_floor * std_floor, mask, tb, error, mahalanobis, (unsigned long long*)counts, rel_ipart, rel_fpart, ipart,
                       fpart);
    hipLaunchKernelGGL(structure_fold_kernel<TruthReliability>, dim3(R, 1), dim3(kBlock), 0, st, rel_ipart, rel_fpart, blocks, R,
                       (int64_t)0, rel_ints, rel_floats);
    hipLaunchKernelGGL(summary_reduce_kernel<TruthSummary>, dim3(1), dim3(kBlock), 0, st, ipart, fpart, blocks, isummary, fsummary);
}

}  // namespace irs
