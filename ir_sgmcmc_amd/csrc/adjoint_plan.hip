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
//
// Sparse data stage: the same three kernels, with the tile and the reach passed in (adjoint_plan.h: PlanShape), on the extents of
// the fixed MASK (mask_extent_kernel).  g_warped is zero further than 2 S from the mask (S = lcc_s: the two box adjoints of the data
// term), z and sigma_M are only used within S of it, the warped image within 3 S:
//   data term   32 x 16 tile columns at reach 2 S, pieces + fills that cover the rest of every column (list 0)
//   LCC map     32 x 16 tile columns at reach S, pieces only (list 1)
//   warp        64 x 8 tile-planes inside the hull at reach 3 S (SSD: 0)
#include "adjoint_plan.h"

#include "kernels.h"

namespace irs {

constexpr int kExtChunk = 32;  // planes one thread of the extent kernel scans

// T = float: g_warped (NaN counts as a gradient); T = uint8_t: the mask
template <typename T>
__device__ __forceinline__ void extent_body(const T* __restrict__ g, int* __restrict__ ext, const Vol& vol) {
    const int x = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6);
    const int nch = (vol.D + kExtChunk - 1) / kExtChunk;
    const int chain = (int)blockIdx.z / nch, za = ((int)blockIdx.z - chain * nch) * kExtChunk, zb = min(za + kExtChunk, vol.D);
    if (x >= vol.W || y >= vol.H) return;
    const int64_t plane = (int64_t)vol.H * vol.W;
    const T* __restrict__ p = g + (int64_t)chain * vol.V + (int64_t)y * vol.W + x;
    int lo = vol.D, hi = -1;
#pragma unroll 8
    for (int z = za; z < zb; ++z) {
        const bool nz = p[z * plane] != (T)0;
        lo = nz ? min(lo, z) : lo;
        hi = nz ? z : hi;
    }
    if (hi < 0) return;
    int* e = ext + ((int64_t)chain * plane + (int64_t)y * vol.W + x) * 2;
    atomicMax(e, vol.D - lo);
    atomicMax(e + 1, hi + 1);
}
__global__ __launch_bounds__(kBlock) void grad_extent_kernel(const float* __restrict__ g, int* __restrict__ ext, Vol vol) {
    extent_body<float>(g, ext, vol);
}
__global__ __launch_bounds__(kBlock) void mask_extent_kernel(const uint8_t* __restrict__ mask, int* __restrict__ ext, Vol vol) {
    extent_body<uint8_t>(mask, ext, vol);
}
static void launch_extent(const float* g, const uint8_t* mask, int* ext, int chains, Vol vol, hipStream_t st) {
    (void)hipMemsetAsync(ext, 0, sizeof(int) * 2 * (size_t)chains * vol.H * vol.W, st);
    const int nch = (vol.D + kExtChunk - 1) / kExtChunk;
    const dim3 grid((unsigned)((vol.W + 63) / 64), (unsigned)((vol.H + 3) / 4), (unsigned)(nch * chains));
    if (g) hipLaunchKernelGGL(grad_extent_kernel, grid, dim3(kBlock), 0, st, g, ext, vol);
    else hipLaunchKernelGGL(mask_extent_kernel, grid, dim3(kBlock), 0, st, mask, ext, vol);
}

// rule 5 of the plan: a chain is marched sparsely only if EVERY step of it belongs to the radius-1 kernel (the same test as
// exp_bwd_march_tile's `hs`, on the bounds the forward pass has just written).  No bounds (the data stage): never dense.
__device__ __forceinline__ bool chain_is_dense(const unsigned* __restrict__ dmax, int chain, int C, int no_steps) {
    bool dense = false;
    if (!dmax) return false;
    for (int k = 0; k < no_steps; ++k) {
        const unsigned* b = dmax + ((int64_t)k * C + chain) * 4;
        const float m = fmaxf(fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1])), __uint_as_float(b[2]));
        dense |= !(m < 1.0f);  // floor(m) + 1 != 1 (or no usable bound)
    }
    return dense;
}

// one wavefront per (tile column of a chain, list); ext_chains == 1: one extent table for every chain
__global__ __launch_bounds__(kWave) void plan_runs_kernel(const int* __restrict__ ext, int ext_chains, const unsigned* __restrict__ dmax,
                                                          int* __restrict__ runs, Vol vol, int C, int no_steps, int ntx, int nty,
                                                          PlanShape shape) {
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
    const int m = plan_reach(shape, k);
    int x0, x1, y0, y1;
    plan_tile_window(tx, shape.tx, m, vol.W, x0, x1);
    plan_tile_window(ty, shape.ty, m, vol.H, y0, y1);
    const int nx = x1 - x0, n = nx * (y1 - y0);
    const int* __restrict__ e = ext + (int64_t)(ext_chains == 1 ? 0 : chain) * vol.H * vol.W * 2;
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

// one workgroup per list (the adjoint: per step).  List order: piece index (z band) outermost, then chain, tile row, tile --
// x-neighbouring tiles of one z band are consecutive; the fills behind the run pieces.  The column plans are formed once (the
// adjoint: nine neighbour look-ups each) and kept in `colplan` for the passes that follow.
__global__ __launch_bounds__(kPlanBlock) void plan_lists_kernel(const int* __restrict__ runs, const unsigned* __restrict__ dmax,
                                                                ColPlan* __restrict__ colplan, PlanEntry* __restrict__ entries,
                                                                int* __restrict__ count, int* __restrict__ stats, Vol vol, int C,
                                                                int no_steps, int ntx, int nty, int cap, PlanShape shape, int forced_len) {
    __shared__ int pieces[kPlanMaxLen + 1], s_maxlen, s_L, s_nrun, wave_tot[kPlanBlock / kWave];
    __shared__ int s_pieces[IRS_MAX_CHAINS], s_planes[IRS_MAX_CHAINS];
    const int k = (int)blockIdx.x, tiles = ntx * nty, cols = C * tiles, tid = (int)threadIdx.x;
    const int lmax = max(min(kPlanMaxLen, vol.D), 1), lmin = min(shape.lmin, lmax);
    const int fill = plan_fill_of(shape, k);
    ColPlan* __restrict__ cps = colplan + (int64_t)k * cols;
    for (int i = tid; i <= kPlanMaxLen; i += kPlanBlock) pieces[i] = 0;
    if (tid < IRS_MAX_CHAINS) s_pieces[tid] = s_planes[tid] = 0;
    if (tid == 0) s_maxlen = s_nrun = 0;
    __syncthreads();
    for (int col = tid; col < cols; col += kPlanBlock) {
        const ColPlan cp = plan_column_by(runs, k, col, C, ntx, nty, vol.D, fill);
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
    if (tid == 0)
        s_L = forced_len > 0 ? min(max(forced_len, kPlanMinForced), lmax) : plan_pick_len(pieces, plan_resident_of(shape, k), lmin, lmax);
    __syncthreads();
    const int L = s_L, levels = plan_pieces(s_maxlen, L);
    PlanEntry* list = entries + (int64_t)k * cap;
    // The (level, column) pairs in list order -- behind the run levels the fills below, then above the run ranges -- are one stream
    // that the workgroup ranks 1024 at a time, not one level per pass: the short pieces of the data stage make many levels of few
    // columns each (256^3: 128 columns), and a pass is two barriers.
    const int stream = (levels + 2) * cols;
    int base = 0;
    for (int i0 = 0; i0 < stream; i0 += kPlanBlock) {
        const int i = i0 + tid;
        bool flag = false;
        ColPlan cp = {0, 0, 0, 0};
        int np = 0, j = 0, col = 0;
        if (i < stream) {
            j = i / cols;
            col = i - j * cols;
            cp = cps[col];
            np = plan_pieces(cp.hi - cp.lo, L);
            flag = j < levels ? j < np : plan_has_fill(cp, j - levels);
        }
        const unsigned long long runs_here = __ballot(flag && j < levels);
        if ((tid & (kWave - 1)) == 0 && runs_here) atomicAdd(&s_nrun, __popcll(runs_here));
        int total;
        const int pos = base + block_rank(flag, wave_tot, total);
        if (flag && pos < cap) {
            list[pos] = j < levels ? plan_entry(cp, col / tiles, col % tiles, np, j) : plan_fill_entry(cp, col / tiles, col % tiles, j - levels);
            atomicAdd(&s_pieces[col / tiles], 1);
        }
        base += total;
    }
    __syncthreads();
    if (tid == 0) {
        count[2 * k] = min(base, cap);
        count[2 * k + 1] = min(s_nrun, cap);
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
static PlanLayout plan_layout(Vol vol, int C, int no_steps, int tx = kPlanTX, int ty = kPlanTY, bool own_ext = true) {
    PlanLayout l;
    l.ntx = (vol.W + tx - 1) / tx;
    l.nty = (vol.H + ty - 1) / ty;
    const size_t cols = (size_t)C * l.ntx * l.nty;
    l.cap = plan_entries_cap((int)cols, vol.D);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += plan_align(bytes); return o; };
    l.ext = take(own_ext ? sizeof(int) * 2 * (size_t)C * vol.H * vol.W : 0);
    l.runs = take(sizeof(int) * 2 * cols * no_steps);
    l.colplan = take(sizeof(ColPlan) * cols * no_steps);
    l.entries = take(sizeof(PlanEntry) * (size_t)l.cap * no_steps);
    l.count = take(sizeof(int) * 2 * no_steps);
    l.stats = take(sizeof(int) * kPlanStats * (size_t)C * no_steps);
    l.total = off;
    return l;
}

size_t adjoint_plan_bytes(Vol vol, int C, int no_steps) { return plan_layout(vol, C, no_steps).total; }

static AdjointPlan plan_views(char* base, const PlanLayout& l, bool own_ext) {
    AdjointPlan p;
    p.ext = own_ext ? (int*)(base + l.ext) : nullptr;
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
AdjointPlan adjoint_plan_views(char* base, Vol vol, int C, int no_steps) { return plan_views(base, plan_layout(vol, C, no_steps), true); }

void launch_adjoint_plan(const float* g_warped, const unsigned* dmax, const AdjointPlan& plan, int no_steps, int C, Vol vol,
                         int64_t G, int forced_len, hipStream_t st) {
    const int g = (int)(G > 0 ? G : 1024);
    const PlanShape shape{kPlanTX, kPlanTY, no_steps, 1, {kFillNext, kFillNext}, {g, g}, kPlanMinLen};
    launch_extent(g_warped, nullptr, plan.ext, C, vol, st);
    hipLaunchKernelGGL(plan_runs_kernel, dim3((unsigned)(C * plan.ntx * plan.nty), (unsigned)no_steps), dim3(kWave), 0, st, plan.ext, C, dmax,
                       plan.runs, vol, C, no_steps, plan.ntx, plan.nty, shape);
    hipLaunchKernelGGL(plan_lists_kernel, dim3((unsigned)no_steps), dim3(kPlanBlock), 0, st, plan.runs, dmax, plan.colplan, plan.entries, plan.count,
                       plan.stats, vol, C, no_steps, plan.ntx, plan.nty, plan.cap, shape, forced_len);
}

// ------------------------------------------------------------------------------------------------
// sparse forward steps: the lists of all steps from the mask's extent table (the data plan's, formed in front of the forward pass)
// and the reaches the host planned (adjoint_plan.h: plan_forward_reach).  Run pieces only: what a step leaves unwritten is stale
// but finite, and only ever meets a zero weight or a zero gradient.  The views have no extent table of their own.
// ------------------------------------------------------------------------------------------------
size_t forward_plan_bytes(Vol vol, int C, int no_steps) { return plan_layout(vol, C, no_steps, kWarpTX, kWarpTY, false).total; }
AdjointPlan forward_plan_views(char* base, Vol vol, int C, int no_steps) {
    return plan_views(base, plan_layout(vol, C, no_steps, kWarpTX, kWarpTY, false), false);
}
int forward_plan_run_bound(const AdjointPlan& plan, int C, Vol vol, int64_t G, int forced_len) {
    return plan_run_bound(C * plan.ntx * plan.nty, vol.D, (int)(G > 0 ? G : 1024), forced_len);
}
void launch_forward_plan(const int* ext, int ext_chains, const AdjointPlan& plan, const int* width, int S, int no_steps, int C, Vol vol,
                         int64_t G, int forced_len, hipStream_t st) {
    const int g = (int)(G > 0 ? G : 1024);
    PlanShape shape{kWarpTX, kWarpTY, 0, 0, {kFillNone, kFillNone}, {g, g}, kPlanMinLen, no_steps, {}};
    for (int k = 0; k < no_steps && k < kPlanMaxLists; ++k) shape.reach[k] = plan_forward_reach(width, no_steps, S, k);
    hipLaunchKernelGGL(plan_runs_kernel, dim3((unsigned)(C * plan.ntx * plan.nty), (unsigned)no_steps), dim3(kWave), 0, st, ext, ext_chains, nullptr,
                       plan.runs, vol, C, no_steps, plan.ntx, plan.nty, shape);
    hipLaunchKernelGGL(plan_lists_kernel, dim3((unsigned)no_steps), dim3(kPlanBlock), 0, st, plan.runs, nullptr, plan.colplan, plan.entries, plan.count,
                       plan.stats, vol, C, no_steps, plan.ntx, plan.nty, plan.cap, shape, forced_len);
}

// ------------------------------------------------------------------------------------------------
// sparse data stage
// ------------------------------------------------------------------------------------------------
struct DataLayout {
    size_t ext, runs, hull, colplan, entries, count, stats, nll, total;
    int cap, ntx, nty, wtx, wty;
};
static DataLayout data_layout(Vol vol, int C) {
    DataLayout l;
    l.ntx = (vol.W + kLccTX - 1) / kLccTX;
    l.nty = (vol.H + kLccTY - 1) / kLccTY;
    l.wtx = (vol.W + kWarpTX - 1) / kWarpTX;
    l.wty = (vol.H + kWarpTY - 1) / kWarpTY;
    const size_t cols = (size_t)C * l.ntx * l.nty;
    l.cap = plan_entries_cap((int)cols, vol.D);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += plan_align(bytes); return o; };
    l.ext = take(sizeof(int) * 2 * (size_t)C * vol.H * vol.W);
    l.runs = take(sizeof(int) * 2 * cols * 2);
    l.hull = take(sizeof(int) * 2 * (size_t)C * l.wtx * l.wty);
    l.colplan = take(sizeof(ColPlan) * cols * 2);
    l.entries = take(sizeof(PlanEntry) * (size_t)l.cap * 2);
    l.count = take(sizeof(int) * 2 * 2);
    l.stats = take(sizeof(int) * kPlanStats * (size_t)C * 2);
    l.nll = take(sizeof(double) * (size_t)l.cap);
    l.total = off;
    return l;
}

size_t data_plan_bytes(Vol vol, int C) { return data_layout(vol, C).total; }

DataPlan data_plan_views(char* base, Vol vol, int C) {
    const DataLayout l = data_layout(vol, C);
    DataPlan p;
    p.ext = (int*)(base + l.ext);
    p.runs = (int*)(base + l.runs);
    p.hull = (int*)(base + l.hull);
    p.colplan = (ColPlan*)(base + l.colplan);
    p.entries = (PlanEntry*)(base + l.entries);
    p.count = (int*)(base + l.count);
    p.stats = (int*)(base + l.stats);
    p.nll = (double*)(base + l.nll);
    p.cap = l.cap;
    p.ntx = l.ntx;
    p.nty = l.nty;
    p.wtx = l.wtx;
    p.wty = l.wty;
    return p;
}

// resident set a list of the data stage is cut for
static int data_list_resident(int s, bool bwd, int C) {
    const int64_t res = lcc_plan_resident(s, bwd, bwd && C > 1);
    return (int)(res > 0 ? res : 1024);
}
int data_plan_run_bound(const DataPlan& plan, int s, bool bwd, int C, Vol vol) {
    return plan_run_bound(C * plan.ntx * plan.nty, vol.D, data_list_resident(s, bwd, C), plan.forced_len);
}

void launch_data_plan(const uint8_t* mask, int mask_chains, const DataPlan& plan, int s, bool lists, int C, Vol vol, hipStream_t st) {
    launch_extent(nullptr, mask, plan.ext, mask_chains, vol, st);
    // the warp's hull: reach 3 s with the LCC map behind it, the mask itself (s == 0) with the SSD residual
    const PlanShape warp{kWarpTX, kWarpTY, 3 * s, 0, {kFillNone, kFillNone}, {1, 1}, kPlanMinLen};
    hipLaunchKernelGGL(plan_runs_kernel, dim3((unsigned)(C * plan.wtx * plan.wty), 1u), dim3(kWave), 0, st, plan.ext, mask_chains, nullptr,
                       plan.hull, vol, C, 1, plan.wtx, plan.wty, warp);
    if (!lists) return;
    const PlanShape lcc{kLccTX, kLccTY, 2 * s, s, {kFillAll, kFillNone}, {data_list_resident(s, true, C), data_list_resident(s, false, C)},
                        kPlanMinLen};
    hipLaunchKernelGGL(plan_runs_kernel, dim3((unsigned)(C * plan.ntx * plan.nty), 2u), dim3(kWave), 0, st, plan.ext, mask_chains, nullptr,
                       plan.runs, vol, C, 2, plan.ntx, plan.nty, lcc);
    hipLaunchKernelGGL(plan_lists_kernel, dim3(2u), dim3(kPlanBlock), 0, st, plan.runs, nullptr, plan.colplan, plan.entries, plan.count, plan.stats,
                       vol, C, 2, plan.ntx, plan.nty, plan.cap, lcc, plan.forced_len);
}

}  // namespace irs
