// Sparse adjoint plan: which planes the adjoint squaring steps have to march.
//
// The gradient that enters the adjoint is g_warped times d(warped)/d(d_n), and the data terms write g_warped = 0 off the mask.  A
// radius-1 adjoint step (max|d_k| < 1 voxel) moves a gradient by less than one voxel, so the gradient that step k produces is
// exactly zero further than m = no_steps - k voxels (Chebyshev) from the support of g_warped.  Three small launches in front of
// the adjoint turn that into work lists, all on the device and in stream order:
//   grad_extent_kernel   per voxel column (y, x) the z-extent of g_warped != 0 (integer atomic maxima into a zeroed table)
//   plan_runs_kernel     per step and 32 x 8 tile column the run range: the hull of the extents, widened by m, of every voxel
//                        column within m of the tile.  A chain one of whose steps leaves the radius-1 kernel gets full columns.
//   plan_lists_kernel    per step the piece list: every run range cut into equal pieces of at most L planes, L the smallest length
//                        whose list fits one resident set of workgroups; the planes the NEXT step's pieces read around their own
//                        range but this step does not march become zero-fill entries behind the run pieces (the gradient buffers
//                        ping-pong, so those planes hold an earlier transition's values).
// The splitting arithmetic is adjoint_plan.h (also run on the CPU by tests/csrc/adjoint_plan_check.cpp).
#include "adjoint_plan.h"

#include "kernels.h"

namespace irs {

constexpr int kExtChunk = 32;  // planes one thread of the extent kernel scans

__global__ __launch_bounds__(kBlock) void grad_extent_kernel(const float* __restrict__ g, int* __restrict__ ext, Vol vol) {
    const int x = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6);
    const int nch = (vol.D + kExtChunk - 1) / kExtChunk;
    const int chain = (int)blockIdx.z / nch, za = ((int)blockIdx.z - chain * nch) * kExtChunk, zb = min(za + kExtChunk, vol.D);
    if (x >= vol.W || y >= vol.H) return;
    const int64_t plane = (int64_t)vol.H * vol.W;
    const float* __restrict__ p = g + (int64_t)chain * vol.V + (int64_t)y * vol.W + x;
    int lo = vol.D, hi = -1;
#pragma unroll 8
    for (int z = za; z < zb; ++z) {
        const bool nz = p[z * plane] != 0.0f;  // (NaN counts as a gradient)
        lo = nz ? min(lo, z) : lo;
        hi = nz ? z : hi;
    }
    if (hi < 0) return;
    int* e = ext + ((int64_t)chain * plane + (int64_t)y * vol.W + x) * 2;
    atomicMax(e, vol.D - lo);
    atomicMax(e + 1, hi + 1);
}

// rule 5 of the plan: a chain is marched sparsely only if EVERY step of it belongs to the radius-1 kernel (the same test as
// exp_bwd_march_tile's `hs`, on the bounds the forward pass has just written)
__device__ __forceinline__ bool chain_is_dense(const unsigned* __restrict__ dmax, int chain, int C, int no_steps) {
    bool dense = false;
    for (int k = 0; k < no_steps; ++k) {
        const unsigned* b = dmax + ((int64_t)k * C + chain) * 4;
        const float m = fmaxf(fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1])), __uint_as_float(b[2]));
        dense |= !(m < 1.0f);  // floor(m) + 1 != 1 (or no usable bound)
    }
    return dense;
}

// one wavefront per (tile column of a chain, step)
__global__ __launch_bounds__(kWave) void plan_runs_kernel(const int* __restrict__ ext, const unsigned* __restrict__ dmax,
                                                          int* __restrict__ runs, Vol vol, int C, int no_steps, int ntx, int nty) {
    const int col = (int)blockIdx.x, k = (int)blockIdx.y, tiles = ntx * nty;
    const int chain = col / tiles, tile = col - chain * tiles, tx = tile % ntx, ty = tile / ntx;
    int* out = runs + ((int64_t)k * C * tiles + col) * 2;
    if (chain_is_dense(dmax, chain, C, no_steps)) {
        if (threadIdx.x == 0) {
            out[0] = 0;
            out[1] = vol.D;
        }
        return;
    }
    const int m = no_steps - k;
    const int x0 = max(tx * kPlanTX - m, 0), x1 = min(tx * kPlanTX + kPlanTX + m, vol.W);
    const int y0 = max(ty * kPlanTY - m, 0), y1 = min(ty * kPlanTY + kPlanTY + m, vol.H);
    const int nx = x1 - x0, n = nx * (y1 - y0);
    const int* __restrict__ e = ext + (int64_t)chain * vol.H * vol.W * 2;
    int lo = vol.D, hi = 0;
    for (int i = (int)threadIdx.x; i < n; i += kWave) {
        const int yy = i / nx, xx = i - yy * nx;
        const int2 ab = *reinterpret_cast<const int2*>(e + ((int64_t)(y0 + yy) * vol.W + x0 + xx) * 2);
        int l, h;
        plan_widen(ab.x, ab.y, m, vol.D, l, h);
        if (h > l) {
            lo = min(lo, l);
            hi = max(hi, h);
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, kWave));
        hi = max(hi, __shfl_xor(hi, off, kWave));
    }
    if (threadIdx.x == 0) {
        out[0] = hi > lo ? lo : 0;
        out[1] = hi > lo ? hi : 0;
    }
}

constexpr int kPlanBlock = 1024;  // threads of plan_lists_kernel (one workgroup per step: wide, so that a step's columns are one pass)
// rank of this thread's flag among the block's flags (thread order) and their number; two barriers
__device__ __forceinline__ int block_rank(bool flag, int* wave_tot, int& total) {
    const unsigned long long b = __ballot(flag);
    const int lane = (int)threadIdx.x & (kWave - 1), w = (int)threadIdx.x / kWave;
    if (lane == 0) wave_tot[w] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kPlanBlock / kWave; ++i) {
        before += i < w ? wave_tot[i] : 0;
        total += wave_tot[i];
    }
    __syncthreads();
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// one workgroup per step.  List order: piece index (z band) outermost, then chain, tile row, tile -- x-neighbouring tiles of one z
// band are consecutive; the fills behind the run pieces.  The column plans are formed once (nine neighbour look-ups each)
// and kept in `colplan` for the passes that follow.
__global__ __launch_bounds__(kPlanBlock) void plan_lists_kernel(const int* __restrict__ runs, const unsigned* __restrict__ dmax,
                                                                ColPlan* __restrict__ colplan, PlanEntry* __restrict__ entries,
                                                                int* __restrict__ count, int* __restrict__ stats, Vol vol, int C,
                                                                int no_steps, int ntx, int nty, int cap, int G, int forced_len) {
    __shared__ int pieces[kPlanMaxLen + 1], s_maxlen, s_L, wave_tot[kPlanBlock / kWave];
    __shared__ int s_pieces[IRS_MAX_CHAINS], s_planes[IRS_MAX_CHAINS];
    const int k = (int)blockIdx.x, tiles = ntx * nty, cols = C * tiles, tid = (int)threadIdx.x;
    const int lmax = max(min(kPlanMaxLen, vol.D), 1), lmin = min(kPlanMinLen, lmax);
    ColPlan* __restrict__ cps = colplan + (int64_t)k * cols;
    for (int i = tid; i <= kPlanMaxLen; i += kPlanBlock) pieces[i] = 0;
    if (tid < IRS_MAX_CHAINS) s_pieces[tid] = s_planes[tid] = 0;
    if (tid == 0) s_maxlen = 0;
    __syncthreads();
    for (int col = tid; col < cols; col += kPlanBlock) {
        const ColPlan cp = plan_column_of(runs, k, col, C, ntx, nty, vol.D);
        cps[col] = cp;
        const int len = cp.hi - cp.lo;
        if (len > 0) {
            atomicMax(&s_maxlen, len);
            atomicAdd(&s_planes[col / tiles], len);
        }
    }
    __syncthreads();  // (also orders this workgroup's writes of `cps` before its reads below)
    // pieces[L] = pieces of all columns when cut at L: a thread owns one candidate length and every (threads / lengths)-th column
    const int n_len = lmax - lmin + 1, groups = kPlanBlock / n_len;
    if (forced_len <= 0 && tid < groups * n_len) {
        const int L = lmin + tid % n_len;
        int sum = 0;
        for (int col = tid / n_len; col < cols; col += groups) sum += plan_pieces(cps[col].hi - cps[col].lo, L);
        atomicAdd(&pieces[L], sum);
    }
    __syncthreads();
    if (tid == 0) s_L = forced_len > 0 ? min(max(forced_len, kPlanMinForced), lmax) : plan_pick_len(pieces, G, lmin, lmax);
    __syncthreads();
    const int L = s_L, levels = plan_pieces(s_maxlen, L);
    PlanEntry* list = entries + (int64_t)k * cap;
    int base = 0, n_run = 0;
    for (int j = 0; j < levels + 2; ++j)  // behind the run pieces: the fills below, then above the run ranges
        for (int c0 = 0; c0 < cols; c0 += kPlanBlock) {
            const int col = c0 + tid;
            bool flag = false;
            ColPlan cp = {0, 0, 0, 0};
            int np = 0;
            if (col < cols) {
                cp = cps[col];
                np = plan_pieces(cp.hi - cp.lo, L);
                flag = j < levels ? j < np : plan_has_fill(cp, j - levels);
            }
            int total;
            const int pos = base + block_rank(flag, wave_tot, total);
            if (flag && pos < cap) {
                list[pos] = j < levels ? plan_entry(cp, col / tiles, col % tiles, np, j) : plan_fill_entry(cp, col / tiles, col % tiles, j - levels);
                atomicAdd(&s_pieces[col / tiles], 1);
            }
            base += total;
            if (j < levels) n_run = base;
        }
    __syncthreads();
    if (tid == 0) {
        count[2 * k] = min(base, cap);
        count[2 * k + 1] = min(n_run, cap);
    }
    if (tid < C) {
        int* s = stats + ((int64_t)k * C + tid) * kPlanStats;
        s[0] = chain_is_dense(dmax, tid, C, no_steps) ? 0 : 1;
        s[1] = L;
        s[2] = s_pieces[tid];
        s[3] = s_planes[tid];
    }
}

static size_t plan_align(size_t b) { return (b + 255) / 256 * 256; }

struct PlanLayout {
    size_t ext, runs, colplan, entries, count, stats, total;
    int cap, ntx, nty;
};
static PlanLayout plan_layout(Vol vol, int C, int no_steps) {
    PlanLayout l;
    l.ntx = (vol.W + kPlanTX - 1) / kPlanTX;
    l.nty = (vol.H + kPlanTY - 1) / kPlanTY;
    const size_t cols = (size_t)C * l.ntx * l.nty;
    l.cap = plan_entries_cap((int)cols, vol.D);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += plan_align(bytes); return o; };
    l.ext = take(sizeof(int) * 2 * (size_t)C * vol.H * vol.W);
    l.runs = take(sizeof(int) * 2 * cols * no_steps);
    l.colplan = take(sizeof(ColPlan) * cols * no_steps);
    l.entries = take(sizeof(PlanEntry) * (size_t)l.cap * no_steps);
    l.count = take(sizeof(int) * 2 * no_steps);
    l.stats = take(sizeof(int) * kPlanStats * (size_t)C * no_steps);
    l.total = off;
    return l;
}

size_t adjoint_plan_bytes(Vol vol, int C, int no_steps) { return plan_layout(vol, C, no_steps).total; }

AdjointPlan adjoint_plan_views(char* base, Vol vol, int C, int no_steps) {
    const PlanLayout l = plan_layout(vol, C, no_steps);
    AdjointPlan p;
    p.ext = (int*)(base + l.ext);
    p.runs = (int*)(base + l.runs);
    p.colplan = (ColPlan*)(base + l.colplan);
    p.entries = (PlanEntry*)(base + l.entries);
    p.count = (int*)(base + l.count);
    p.stats = (int*)(base + l.stats);
    p.cap = l.cap;
    p.ntx = l.ntx;
    p.nty = l.nty;
    return p;
}

void launch_adjoint_plan(const float* g_warped, const unsigned* dmax, const AdjointPlan& plan, int no_steps, int C, Vol vol,
                         int64_t G, int forced_len, hipStream_t st) {
    (void)hipMemsetAsync(plan.ext, 0, sizeof(int) * 2 * (size_t)C * vol.H * vol.W, st);
    const int nch = (vol.D + kExtChunk - 1) / kExtChunk;
    hipLaunchKernelGGL(grad_extent_kernel, dim3((unsigned)((vol.W + 63) / 64), (unsigned)((vol.H + 3) / 4), (unsigned)(nch * C)), dim3(kBlock),
                       0, st, g_warped, plan.ext, vol);
    hipLaunchKernelGGL(plan_runs_kernel, dim3((unsigned)(C * plan.ntx * plan.nty), (unsigned)no_steps), dim3(kWave), 0, st, plan.ext, dmax,
                       plan.runs, vol, C, no_steps, plan.ntx, plan.nty);
    hipLaunchKernelGGL(plan_lists_kernel, dim3((unsigned)no_steps), dim3(kPlanBlock), 0, st, plan.runs, dmax, plan.colplan, plan.entries, plan.count,
                       plan.stats, vol, C, no_steps, plan.ntx, plan.nty, plan.cap, (int)(G > 0 ? G : 1024), forced_len);
}

}  // namespace irs
