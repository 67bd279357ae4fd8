// Sparse adjoint plan: which planes the adjoint squaring steps have to march.
//
// The gradient that enters the adjoint is g_warped times d(warped)/d(d_n), and the data terms write g_warped = 0 off the mask.  A
// radius-1 adjoint step (max|d_k| < 1 voxel) moves a gradient by less than one voxel, so the gradient that step k produces is
// exactly zero further than m = no_steps - k voxels (Chebyshev) from the support of g_warped.  Small launches in front of
// the adjoint turn that into work lists, all on the device and in stream order:
//   grad_extent_kernel   per voxel column (y, x) the z-extent of g_warped != 0 -- only where the data plan has not formed the MASK's
//                        table in this transition: g_warped lies within 2 S of the mask, and the lists are cut from that table
//   plan_runs_kernel     per step and 32 x 8 tile column the run range: the hull of the extents, widened by m, of every voxel
//                        column within m of the tile.  A chain one of whose steps leaves the radius-1 kernel gets full columns.
//   plan_lists_kernel    per step the piece list: every run range cut into equal pieces of at most L planes, L the smallest length
//                        whose list fits one resident set of workgroups; the planes the NEXT step's pieces read around their own
//                        range but this step does not march become zero-fill entries behind the run pieces (the gradient buffers
//                        ping-pong, so those planes hold an earlier transition's values).
// A list whose inputs did not change since it was cut is left as it is ("plan reuse" below).
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

// ------------------------------------------------------------------------------------------------
// extent pass: one workgroup owns its voxel columns over all of z -- kExtXL lanes along x (the mask: 4 columns each, read as one
// 32-bit word where the rows allow it) times kExtZP parts of z, combined through LDS.  The owning thread compares the column's final
// entry with the one in the table, stores only a changed one, and a workgroup that changed anything advances the table's generation
// (adjoint_plan.h: PlanGen).  No clear and no atomics on entries: the zeroed workspace is a table of empty columns.
// ------------------------------------------------------------------------------------------------
constexpr int kExtXL = 32, kExtZP = kBlock / kExtXL;
static_assert(kBlock == 256 && kExtZP == 8, "extent pass: 32 lanes x 8 parts of z");

// T = float: g_warped, one column per lane (NaN counts as a gradient); T = uint8_t: the mask, CPL = 4 columns per lane
template <typename T, int CPL, bool WORD>
__device__ __forceinline__ void extent_body(const T* __restrict__ g, int* __restrict__ ext, PlanGen* __restrict__ gen, const Vol& vol) {
    __shared__ int s_lo[kExtZP][kExtXL * CPL], s_hi[kExtZP][kExtXL * CPL];
    const int lane = (int)threadIdx.x % kExtXL, part = (int)threadIdx.x / kExtXL;
    const int x0 = ((int)blockIdx.x * kExtXL + lane) * CPL, y = (int)blockIdx.y, chain = (int)blockIdx.z;
    const int per = (vol.D + kExtZP - 1) / kExtZP, za = min(part * per, vol.D), zb = min(za + per, vol.D);
    const int64_t plane = (int64_t)vol.H * vol.W;
    const T* __restrict__ p = g + (int64_t)chain * vol.V + (int64_t)y * vol.W + x0;
    int lo[CPL], hi[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        lo[j] = vol.D;
        hi[j] = -1;
    }
    if (x0 < vol.W) {
#pragma unroll 8
        for (int z = za; z < zb; ++z) {
            if constexpr (WORD) {  // (W % 4 == 0: the four columns are inside the row together)
                const unsigned w = *reinterpret_cast<const unsigned*>(p + z * plane);
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const bool nz = ((w >> (8 * j)) & 0xffu) != 0u;
                    lo[j] = nz ? min(lo[j], z) : lo[j];
                    hi[j] = nz ? z : hi[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < CPL; ++j) {
                    const bool nz = x0 + j < vol.W && p[z * plane + j] != (T)0;
                    lo[j] = nz ? min(lo[j], z) : lo[j];
                    hi[j] = nz ? z : hi[j];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        s_lo[part][lane * CPL + j] = lo[j];
        s_hi[part][lane * CPL + j] = hi[j];
    }
    __syncthreads();
    int changed = 0;
    const int c = (int)threadIdx.x, x = (int)blockIdx.x * kExtXL * CPL + c;
    if (c < kExtXL * CPL && x < vol.W) {
        int l = vol.D, h = -1;
#pragma unroll
        for (int q = 0; q < kExtZP; ++q) {
            l = min(l, s_lo[q][c]);
            h = max(h, s_hi[q][c]);
        }
        int a, b;
        plan_extent_entry(l, h, vol.D, a, b);
        int2* e = reinterpret_cast<int2*>(ext + ((int64_t)chain * plane + (int64_t)y * vol.W + x) * 2);
        const int2 old = *e;
        if (old.x != a || old.y != b) {
            *e = make_int2(a, b);
            changed = 1;
        }
    }
    if (__syncthreads_or(changed) && threadIdx.x == 0) atomicAdd(gen, (PlanGen)1);
}
__global__ __launch_bounds__(kBlock) void grad_extent_kernel(const float* __restrict__ g, int* __restrict__ ext, PlanGen* __restrict__ gen, Vol vol) {
    extent_body<float, 1, false>(g, ext, gen, vol);
}
template <bool WORD>
__global__ __launch_bounds__(kBlock) void mask_extent_kernel(const uint8_t* __restrict__ mask, int* __restrict__ ext, PlanGen* __restrict__ gen, Vol vol) {
    extent_body<uint8_t, 4, WORD>(mask, ext, gen, vol);
}
static void launch_extent(const float* g, const uint8_t* mask, int* ext, PlanGen* gen, int chains, Vol vol, hipStream_t st) {
    const int cols = kExtXL * (g ? 1 : 4);
    const dim3 grid((unsigned)((vol.W + cols - 1) / cols), (unsigned)vol.H, (unsigned)chains);
    if (g) hipLaunchKernelGGL(grad_extent_kernel, grid, dim3(kBlock), 0, st, g, ext, gen, vol);
    else if (vol.W % 4 == 0 && (uintptr_t)mask % 4 == 0) hipLaunchKernelGGL(mask_extent_kernel<true>, grid, dim3(kBlock), 0, st, mask, ext, gen, vol);
    else hipLaunchKernelGGL(mask_extent_kernel<false>, grid, dim3(kBlock), 0, st, mask, ext, gen, vol);
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

// ------------------------------------------------------------------------------------------------
// plan reuse.  A family is the lists one marching kernel (or the warp: its hull, run ranges only) takes from one extent table; a
// batch is the families one pair of launches cuts.  Every workgroup of the runs stage and the single workgroup per list of the
// lists stage evaluate the same predicate (adjoint_plan.h: plan_reusable) on the same data -- the list's record, which only the
// lists stage writes, behind the runs stage in stream order -- and leave at once when it holds.
// ------------------------------------------------------------------------------------------------
struct PlanFamily {
    const int* ext;
    const PlanGen* gen;
    const unsigned* dmax;  // the adjoint: bounds of d_k, [no_steps][C][4]; else nullptr
    int* runs;             // [lists][C tiles][2] (the hull: the warp's table itself)
    ColPlan* colplan;
    PlanEntry* entries;
    int* count;
    int* stats;
    PlanRecord* rec;       // [lists]
    int* counters;         // the family's {rebuilds, reuses}
    int lists, ntx, nty, cap, forced_len, ext_chains, source, no_steps, runs_only;
    PlanShape shape;
};
constexpr int kBatchFamilies = 3;
struct PlanBatch {
    PlanFamily f[kBatchFamilies];
    int nf, reuse;
};

__device__ __forceinline__ unsigned dense_mask(const unsigned* __restrict__ dmax, int C, int no_steps) {
    unsigned m = 0;
    for (int c = 0; c < C; ++c) m |= chain_is_dense(dmax, c, C, no_steps) ? 1u << c : 0u;
    return m;
}
// blockIdx -> family and list; false: beyond the batch
__device__ __forceinline__ bool batch_list(const PlanBatch& b, int id, int& fi, int& k) {
    fi = 0;
    k = id;
    while (fi < b.nf && k >= b.f[fi].lists) k -= b.f[fi++].lists;
    return fi < b.nf;
}
__device__ __forceinline__ bool list_reusable(const PlanFamily& f, int k, int C, const Vol& vol, int reuse, PlanKey& key, unsigned& dense,
                                              PlanGen& gen) {
    key = plan_key(f.shape, k, f.lists, f.forced_len, C, f.ext_chains, vol.D, vol.H, vol.W, f.source, f.dmax != nullptr);
    dense = dense_mask(f.dmax, C, f.no_steps);
    gen = *f.gen;
    return reuse != 0 && plan_reusable(f.rec[k], key, dense, gen);
}

// one wavefront per (tile column of a chain, list); ext_chains == 1: one extent table for every chain
__global__ __launch_bounds__(kWave) void plan_runs_kernel(PlanBatch batch, Vol vol, int C) {
    int fi, k;
    if (!batch_list(batch, (int)blockIdx.y, fi, k)) return;
    const PlanFamily& f = batch.f[fi];
    const int col = (int)blockIdx.x, ntx = f.ntx, tiles = ntx * f.nty;
    if (col >= C * tiles) return;
    PlanKey key;
    unsigned dense;
    PlanGen gen;
    if (list_reusable(f, k, C, vol, batch.reuse, key, dense, gen)) return;
    const int chain = col / tiles, tile = col - chain * tiles, tx = tile % ntx, ty = tile / ntx;
    int* out = f.runs + ((int64_t)k * C * tiles + col) * 2;
    if (dense >> chain & 1u) {
        if (threadIdx.x == 0) {
            out[0] = 0;
            out[1] = vol.D;
        }
        return;
    }
    const int m = plan_reach(f.shape, k);
    int x0, x1, y0, y1;
    plan_tile_window(tx, f.shape.tx, m, vol.W, x0, x1);
    plan_tile_window(ty, f.shape.ty, m, vol.H, y0, y1);
    const int nx = x1 - x0, n = nx * (y1 - y0);
    const int* __restrict__ e = f.ext + (int64_t)(f.ext_chains == 1 ? 0 : chain) * vol.H * vol.W * 2;
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
// A list whose record still holds is left as it is (its `count` and `stats` rows with it); a rebuilt one gets its record here, by
// the only workgroup that writes it.  The hull (runs_only) has no list: its workgroup only keeps the record.
__global__ __launch_bounds__(kPlanBlock) void plan_lists_kernel(PlanBatch batch, Vol vol, int C) {
    __shared__ int pieces[kPlanMaxLen + 1], s_maxlen, s_L, s_nrun, wave_tot[kPlanBlock / kWave];
    __shared__ int s_pieces[IRS_MAX_CHAINS], s_planes[IRS_MAX_CHAINS];
    int fi, k;
    if (!batch_list(batch, (int)blockIdx.x, fi, k)) return;
    const PlanFamily& f = batch.f[fi];
    const int tid = (int)threadIdx.x;
    PlanKey key;
    unsigned dense;
    PlanGen gen;
    const bool keep = list_reusable(f, k, C, vol, batch.reuse, key, dense, gen);
    if (tid == 0) atomicAdd(f.counters + (keep ? 1 : 0), 1);
    if (keep) return;
    if (f.runs_only) {
        if (tid == 0) f.rec[k] = plan_record(key, dense, gen);
        return;
    }
    const int* __restrict__ runs = f.runs;
    PlanEntry* __restrict__ entries = f.entries;
    int* __restrict__ count = f.count;
    int* __restrict__ stats = f.stats;
    const PlanShape& shape = f.shape;
    const int ntx = f.ntx, nty = f.nty, cap = f.cap, forced_len = f.forced_len;
    const int tiles = ntx * nty, cols = C * tiles;
    const int lmax = max(min(kPlanMaxLen, vol.D), 1), lmin = min(shape.lmin, lmax);
    const int fill = plan_fill_of(shape, k);
    ColPlan* __restrict__ cps = f.colplan + (int64_t)k * cols;
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
        f.rec[k] = plan_record(key, dense, gen);
    }
    if (tid < C) {
        int* s = stats + ((int64_t)k * C + tid) * kPlanStats;
        s[0] = dense >> tid & 1u ? 0 : 1;
        s[1] = L;
        s[2] = s_pieces[tid];
        s[3] = s_planes[tid];
    }
}

static size_t plan_align(size_t b) { return (b + 255) / 256 * 256; }

struct PlanLayout {
    size_t ext, runs, colplan, entries, count, stats, rec, gen, counters, total;
    int cap, ntx, nty;
};
constexpr size_t kCounterBytes = sizeof(int) * 2;  // {rebuilds, reuses} of a family
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
    l.rec = take(sizeof(PlanRecord) * (size_t)no_steps);
    l.gen = take(own_ext ? sizeof(PlanGen) : 0);
    l.counters = take(kCounterBytes);
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
    p.rec = (PlanRecord*)(base + l.rec);
    p.gen = own_ext ? (PlanGen*)(base + l.gen) : nullptr;
    p.counters = (int*)(base + l.counters);
    p.cap = l.cap;
    p.ntx = l.ntx;
    p.nty = l.nty;
    return p;
}
AdjointPlan adjoint_plan_views(char* base, Vol vol, int C, int no_steps) { return plan_views(base, plan_layout(vol, C, no_steps), true); }

// the lists of `plan`, cut from the table (ext, gen) of ext_chains chains
static PlanFamily list_family(const AdjointPlan& plan, const int* ext, const PlanGen* gen, int ext_chains, int source, const unsigned* dmax,
                              int lists, int forced_len, const PlanShape& shape) {
    PlanFamily f{};
    f.ext = ext;
    f.gen = gen;
    f.dmax = dmax;
    f.runs = plan.runs;
    f.colplan = plan.colplan;
    f.entries = plan.entries;
    f.count = plan.count;
    f.stats = plan.stats;
    f.rec = plan.rec;
    f.counters = plan.counters;
    f.lists = lists;
    f.ntx = plan.ntx;
    f.nty = plan.nty;
    f.cap = plan.cap;
    f.forced_len = forced_len;
    f.ext_chains = ext_chains;
    f.source = source;
    f.no_steps = lists;
    f.shape = shape;
    return f;
}
// the runs launch and the lists launch of a batch
static void launch_batch(PlanBatch& b, int C, Vol vol, int reuse, hipStream_t st) {
    int cols = 0, lists = 0;
    for (int i = 0; i < b.nf; ++i) {
        cols = plan_max(cols, C * b.f[i].ntx * b.f[i].nty);
        lists += b.f[i].lists;
    }
    b.reuse = reuse & 1;
    hipLaunchKernelGGL(plan_runs_kernel, dim3((unsigned)cols, (unsigned)lists), dim3(kWave), 0, st, b, vol, C);
    hipLaunchKernelGGL(plan_lists_kernel, dim3((unsigned)lists), dim3(kPlanBlock), 0, st, b, vol, C);
}

void launch_adjoint_plan(const float* g_warped, const DataPlan* mask_table, int mask_chains, int S, const unsigned* dmax, const AdjointPlan& plan,
                         int no_steps, int C, Vol vol, int64_t G, int forced_len, int reuse, hipStream_t st) {
    const int g = (int)(G > 0 ? G : 1024);
    const int source = mask_table ? kSourceMask : kSourceGradient;
    const PlanShape shape{kPlanTX, kPlanTY, plan_adjoint_reach0(no_steps, S, source), 1, {kFillNext, kFillNext}, {g, g}, kPlanMinLen};
    if (!mask_table) launch_extent(g_warped, nullptr, plan.ext, plan.gen, C, vol, st);
    PlanBatch b{};
    b.nf = 1;
    b.f[0] = mask_table ? list_family(plan, mask_table->ext, mask_table->gen, mask_chains, source, dmax, no_steps, forced_len, shape)
                        : list_family(plan, plan.ext, plan.gen, C, source, dmax, no_steps, forced_len, shape);
    launch_batch(b, C, vol, reuse, st);
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
// ------------------------------------------------------------------------------------------------
// sparse data stage
// ------------------------------------------------------------------------------------------------
struct DataLayout {
    size_t ext, runs, hull, colplan, entries, count, stats, nll, rec, gen, counters, total;
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
    l.rec = take(sizeof(PlanRecord) * 3);
    l.gen = take(sizeof(PlanGen));
    l.counters = take(kCounterBytes);
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
    p.rec = (PlanRecord*)(base + l.rec);
    p.gen = (PlanGen*)(base + l.gen);
    p.counters = (int*)(base + l.counters);
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

// Everything in front of the forward pass, three launches: the mask's extent pass, then one runs and one lists launch over the warp's
// hull (its record alone in the lists stage), the two lists of the LCC kernels (`lists`) and the forward steps' lists (`fplan`, with
// the widths the host planned; nullptr: dense forward steps).  Records: DataPlan::rec[0 .. 1] the lists, [2] the hull.
void launch_front_plans(const uint8_t* mask, int mask_chains, const DataPlan& plan, int s, bool lists, const AdjointPlan* fplan, const int* width,
                        int no_steps, int64_t fwd_G, int fwd_forced, int C, Vol vol, int reuse, hipStream_t st) {
    launch_extent(nullptr, mask, plan.ext, plan.gen, mask_chains, vol, st);
    PlanBatch b{};
    // the warp's hull: reach 3 s with the LCC map behind it, the mask itself (s == 0) with the SSD residual
    PlanFamily& hull = b.f[b.nf++];
    hull.ext = plan.ext;
    hull.gen = plan.gen;
    hull.runs = plan.hull;
    hull.rec = plan.rec + 2;
    hull.counters = plan.counters;
    hull.lists = hull.no_steps = hull.runs_only = 1;
    hull.ntx = plan.wtx;
    hull.nty = plan.wty;
    hull.ext_chains = mask_chains;
    hull.source = kSourceMask;
    hull.shape = PlanShape{kWarpTX, kWarpTY, 3 * s, 0, {kFillNone, kFillNone}, {1, 1}, kPlanMinLen};
    if (lists) {
        PlanFamily& f = b.f[b.nf++];
        f = hull;
        f.runs = plan.runs;
        f.colplan = plan.colplan;
        f.entries = plan.entries;
        f.count = plan.count;
        f.stats = plan.stats;
        f.rec = plan.rec;
        f.lists = f.no_steps = 2;
        f.runs_only = 0;
        f.ntx = plan.ntx;
        f.nty = plan.nty;
        f.cap = plan.cap;
        f.forced_len = plan.forced_len;
        f.shape = PlanShape{kLccTX, kLccTY, 2 * s, s, {kFillAll, kFillNone}, {data_list_resident(s, true, C), data_list_resident(s, false, C)},
                            kPlanMinLen};
    }
    if (fplan) {
        const int g = (int)(fwd_G > 0 ? fwd_G : 1024);
        PlanShape shape{kWarpTX, kWarpTY, 0, 0, {kFillNone, kFillNone}, {g, g}, kPlanMinLen, no_steps, {}};
        for (int k = 0; k < no_steps && k < kPlanMaxLists; ++k) shape.reach[k] = plan_forward_reach(width, no_steps, s, k);
        b.f[b.nf++] = list_family(*fplan, plan.ext, plan.gen, mask_chains, kSourceMask, nullptr, no_steps, fwd_forced, shape);
    }
    launch_batch(b, C, vol, reuse, st);
}

}  // namespace irs
