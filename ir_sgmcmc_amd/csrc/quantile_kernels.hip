// Displacement credible intervals (absent in the reference): per voxel and channel a histogram of the displacement over the
// recorded samples, uint16 counts, bin-major (3,B,V), around the displacement of the first record; at the end the quantiles
// of given probabilities, the width of the band between the first and the last, and its summary.
//
//  - update: one launch per recorded step for all C chains, one voxel per thread on the 64 x 4 voxel grid of the pointwise
//    kernels, compiled per C so the chains' bins stay in registers.  The thread works out the 3 C bins, then, per channel,
//    lets the first chain of each distinct bin carry the count of all chains in it: the loads of all those counts are issued
//    before the first store (the addresses are distinct), and a count is read and written once however many chains share it.
//    Neighbouring lanes mostly hit the same bin plane (x - centre is smooth), so a wavefront's 2-byte accesses share cache
//    lines.  Each thread owns its voxel: plain read-modify-writes, no atomics.  The first record of all writes the centre and
//    every bin of the voxel and reads no state.
//  - finalize: a grid-stride stream over voxels walks the B planes of each channel (coalesced reads, 16 planes loaded ahead
//    of their use), compares the running count with the next pending integer threshold ceil(p n) (cum >= p n exactly when
//    cum >= ceil(p n), and the thresholds are sorted), interpolates in double where a threshold is crossed, and writes the
//    P x 3 quantile planes and the width plane; the summary over the mask stays in registers and is reduced by
//    summary_device.h.
#include "kernels.h"
#include "quantile_device.h"
#include "summary_device.h"

namespace irs {
namespace {

// the summary columns: integer sums over the mask {voxels, voxels with an out-of-range quantile, samples in the two
// open-ended bins}; then doubles over the stored float32 maps of the in-range masked voxels {sum ci_width, max ci_width,
// sum of the per-channel widths x, y, z}.  The maximum never sees a NaN.
struct QuantileSummary {
    static constexpr int kInts = IRS_QUANTILE_SUMMARY_INTS, kFloats = IRS_QUANTILE_SUMMARY_FLOATS;
    static constexpr Col kind(int j) { return j == 1 ? Col::Max : Col::Sum; }
};
using QAcc = SummaryAcc<QuantileSummary>;
constexpr int kQMaxProbs = IRS_QUANTILE_MAX_PROBS;
constexpr int kQBatch = 16;  // bin planes a finalize thread loads before it uses the first

struct QInvWidth {
    float w[3];
};

// x (C,3,V) float32; centre (3,V) float32; hist (3,B,V) uint16.  One voxel per thread.
template <int C>
__global__ __launch_bounds__(kBlock) void quantile_update_kernel(const float* __restrict__ x, float* __restrict__ centre,
                                                                 uint16_t* __restrict__ hist, int B, QInvWidth iw,
                                                                 int records_before, Vol vol) {
    IRS_VOXEL(vol, plane_, xx_, yy_, zz_, p);
    (void)plane_;
    const bool fresh = records_before == 0;  // the first record of all: the state is written, never read
    int bin[3][C];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float c0;
        if (fresh) {
            c0 = x[a * vol.V + p];
            centre[a * vol.V + p] = c0;
        } else {
            c0 = centre[a * vol.V + p];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) bin[a][c] = quantile_bin(x[(int64_t)(c * 3 + a) * vol.V + p], c0, iw.w[a], B);
    }
    if (fresh) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            uint16_t* h = hist + (int64_t)a * B * vol.V + p;
            for (int b = 0; b < B; ++b) {
                int k = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) k += bin[a][c] == b;
                h[(int64_t)b * vol.V] = (uint16_t)k;
            }
        }
        return;
    }
    int add[3][C];  // chains in the bin of chain c, at the first chain of that bin; 0 at the others
    uint16_t old[3][C];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            bool first = true;
            int k = 0;
#pragma unroll
            for (int e = 0; e < C; ++e) {
                const bool same = bin[a][e] == bin[a][c];
                if (e < c) first = first && !same;
                if (e >= c) k += same;
            }
            add[a][c] = first ? k : 0;
            old[a][c] = 0;
            if (add[a][c]) old[a][c] = hist[((int64_t)a * B + bin[a][c]) * vol.V + p];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (add[a][c]) hist[((int64_t)a * B + bin[a][c]) * vol.V + p] = (uint16_t)(old[a][c] + add[a][c]);
    }
}

struct QParams {
    double r[kQMaxProbs];  // p n
    int kth[kQMaxProbs];   // ceil(p n): the running count reaches r exactly when it reaches this
    double width[3], scale[3];
    int P, B;
};

// centre (3,V), hist (3,B,V) after n records -> quantiles (P,3,V), ci_width (V) float32 and, per block, the summary columns
__global__ __launch_bounds__(kBlock) void quantile_finalize_kernel(const float* __restrict__ centre, const uint16_t* __restrict__ hist,
                                                                   int64_t V, QParams prm, const uint8_t* __restrict__ mask,
                                                                   float* __restrict__ quantiles, float* __restrict__ ci_width,
                                                                   long long* __restrict__ ipart, double* __restrict__ fpart) {
    __shared__ QAcc smem[QAcc::kG];
    QAcc acc = QAcc::identity();
    const int B = prm.B, P = prm.P;
    const float nan = __builtin_nanf("");
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < V; v += (int64_t)gridDim.x * kBlock) {
        bool bad = false;
        int clipped = 0;
        double wa[3] = {0.0, 0.0, 0.0};  // |q_last - q_first| per channel, from the stored float32 values
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint16_t* h = hist + (int64_t)a * B * V + v;
            const double c0 = (double)centre[a * V + v];
            // the thresholds are non-decreasing, so the pending ones are j >= jn and only the next one is compared in the loop
            int jn = 0, knext = prm.kth[0], cum = 0;
            float qf = nan, ql = nan;
            for (int b0 = 0; b0 < B; b0 += kQBatch) {
                int cnt[kQBatch];  // a batch of planes is loaded before any is used: kQBatch loads in flight per channel
#pragma unroll
                for (int i = 0; i < kQBatch; ++i) cnt[i] = b0 + i < B ? (int)h[(int64_t)(b0 + i) * V] : 0;
#pragma unroll
                for (int i = 0; i < kQBatch; ++i) {
                    const int b = b0 + i, prev = cum;
                    cum += cnt[i];
                    clipped += (b == 0 || b == B - 1) ? cnt[i] : 0;
                    while (cum >= knext) {  // rare: P times per channel
                        double r = 0.0;
#pragma unroll
                        for (int j = 0; j < kQMaxProbs; ++j) r = j == jn ? prm.r[j] : r;
                        const float qv = quantile_value(c0, b, B, r, prev, cnt[i], prm.width[a], prm.scale[a]);
                        quantiles[((int64_t)jn * 3 + a) * V + v] = qv;
                        bad = bad || qv != qv;
                        qf = jn == 0 ? qv : qf;
                        ql = jn == P - 1 ? qv : ql;
                        ++jn;
                        knext = INT32_MAX;  // nothing pending: no count reaches it
#pragma unroll
                        for (int j = 1; j < kQMaxProbs; ++j) knext = (j == jn && j < P) ? prm.kth[j] : knext;
                    }
                }
            }
            for (; jn < P; ++jn) {  // a state that holds fewer than n records: nothing to report
                quantiles[((int64_t)jn * 3 + a) * V + v] = nan;
                bad = true;
            }
            wa[a] = fabs((double)ql - (double)qf);
        }
        const float w = bad ? nan : (float)sqrt(wa[0] * wa[0] + wa[1] * wa[1] + wa[2] * wa[2]);
        ci_width[v] = w;
        if (!mask || mask[v]) {
            acc.i[0] += 1;
            acc.i[2] += clipped;
            if (bad) {
                acc.i[1] += 1;
            } else {
                acc.f[0] += (double)w;
                acc.f[1] = fmax(acc.f[1], (double)w);
                acc.f[2] += wa[0];
                acc.f[3] += wa[1];
                acc.f[4] += wa[2];
            }
        }
    }
    acc.block_reduce(smem);
    if (threadIdx.x == 0) acc.store(ipart, fpart, blockIdx.x);
}

template <int C>
void launch_update(const float* x, float* centre, uint16_t* hist, int B, QInvWidth iw, int records_before, Vol vol, hipStream_t st) {
    hipLaunchKernelGGL(quantile_update_kernel<C>, vox_grid(vol, 1), dim3(kBlock), 0, st, x, centre, hist, B, iw, records_before, vol);
}

}  // namespace

void launch_quantile_update(const float* x, int C, float* centre, uint16_t* hist, int bins, const float* inv_width,
                            int records_before, Vol vol, hipStream_t st) {
    static_assert(IRS_MAX_CHAINS == 8, "one instantiation per chain count");
    const QInvWidth iw{{inv_width[0], inv_width[1], inv_width[2]}};
    switch (C) {
        case 1: launch_update<1>(x, centre, hist, bins, iw, records_before, vol, st); break;
        case 2: launch_update<2>(x, centre, hist, bins, iw, records_before, vol, st); break;
        case 3: launch_update<3>(x, centre, hist, bins, iw, records_before, vol, st); break;
        case 4: launch_update<4>(x, centre, hist, bins, iw, records_before, vol, st); break;
        case 5: launch_update<5>(x, centre, hist, bins, iw, records_before, vol, st); break;
        case 6: launch_update<6>(x, centre, hist, bins, iw, records_before, vol, st); break;
        case 7: launch_update<7>(x, centre, hist, bins, iw, records_before, vol, st); break;
        default: launch_update<8>(x, centre, hist, bins, iw, records_before, vol, st); break;
    }
}

void launch_quantile_finalize(const float* centre, const uint16_t* hist, int bins, int64_t V, int n, const float* width,
                              const float* scale, const double* probs, int P, const uint8_t* mask, float* quantiles,
                              float* ci_width, long long* isummary, double* fsummary, void* ws, hipStream_t st) {
    const SummaryPartials<QuantileSummary> part(V, ws, IRS_QUANTILE_WS_BYTES);
    QParams prm{};
    for (int j = 0; j < kQMaxProbs; ++j) {
        prm.r[j] = j < P ? probs[j] * (double)n : 0.0;
        prm.kth[j] = j < P ? (int)ceil(prm.r[j]) : 0;
    }
    for (int a = 0; a < 3; ++a) {
        prm.width[a] = (double)width[a];
        prm.scale[a] = (double)scale[a];
    }
    prm.P = P;
    prm.B = bins;
    hipLaunchKernelGGL(quantile_finalize_kernel, dim3(part.blocks), dim3(kBlock), 0, st, centre, hist, V, prm, mask, quantiles,
                       ci_width, part.ipart, part.fpart);
    part.reduce(isummary, fsummary, st);
}

}  // namespace irs
