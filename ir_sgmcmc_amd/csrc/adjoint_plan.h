// Splitting arithmetic of the sparse plans (adjoint_plan.hip): which planes of a tile column an adjoint squaring step -- or a kernel
// of the data stage -- marches, which it only zero-fills, and how a column is cut into pieces.  Plain integer functions, host and
// device: the device kernels and tests/csrc/adjoint_plan_check.cpp / data_plan_check.cpp (CPU programs) run the same code.
#pragma once

#if defined(__HIPCC__)
#define IRS_HD __host__ __device__ inline
#else
#define IRS_HD inline
#endif

namespace irs {

#ifndef IRS_MTX
#define IRS_MTX 32
#define IRS_MTY 8
#endif
constexpr int kPlanTX = IRS_MTX, kPlanTY = IRS_MTY;  // the adjoint's tile column (exp_kernels.hip: MTX x MTY)
#ifndef IRS_BWD_MAX_SEG
#define IRS_BWD_MAX_SEG 64  // longest z-segment of the adjoint step (exp_kernels.hip)
#endif
constexpr int kPlanMaxLen = IRS_BWD_MAX_SEG;
constexpr int kPlanMinLen = 8;     // shortest piece the length search may choose (two run-in planes per piece: 25 % at 8)
constexpr int kPlanMinForced = 4;  // shortest piece a forced length (march_seg) may ask for; sizes the entry lists
constexpr int kPlanStats = 4;      // per (step, chain): engaged, piece length, pieces, planes in run ranges
constexpr int kForwardStats = 5;   // read-back of the sparse forward steps: the four above and the step's planned width

// One unit of work of a step, on the planes [z0, z1) of tile column `tile` of `chain`: march them (fill == 0) or store zeros to them.
// Marching and filling are separate entries: a workgroup that did both kept the fill's addresses alive across the tile body, and
// the radius-1 kernel, which sits exactly at 128 VGPRs, then needed scratch memory -- 11 % slower per plane step.
struct PlanEntry {
    int chain, tile, z0, z1, fill, pad;
};

// A tile column of one step: run range [lo, hi) (empty: lo == hi) inside the written range [f0, f1).
struct ColPlan {
    int lo, hi, f0, f1;
};

IRS_HD int plan_min(int a, int b) { return a < b ? a : b; }
IRS_HD int plan_max(int a, int b) { return a > b ? a : b; }

// z-extent of one voxel column widened by the reach m of a step and clipped to the volume; (0, 0) if the column is empty.
// The extent table holds (D - lo, hi) per column, both 0 for an empty one (integer maxima of a zeroed table).
IRS_HD void plan_widen(int a, int b, int m, int D, int& lo, int& hi) {
    lo = hi = 0;
    if (b <= 0) return;
    lo = plan_max(D - a - m, 0);
    hi = plan_min(b + m, D);
}

// run range and what the next step reads of this column (`need`, empty: nlo >= nhi) -> the column's plan
IRS_HD ColPlan plan_column(int lo, int hi, int nlo, int nhi) {
    const bool run = hi > lo, need = nhi > nlo;
    if (!run) return need ? ColPlan{nhi, nhi, nlo, nhi} : ColPlan{0, 0, 0, 0};
    return ColPlan{lo, hi, need ? plan_min(lo, nlo) : lo, need ? plan_max(hi, nhi) : hi};
}

// The plan of tile column `col` (chain-major, then tile row, tile) of step k from the run ranges runs[step][column][2]: its own run
// range and what step k - 1 reads of it -- the pieces of the column and of its 8 neighbours reach one plane beyond their own range
// (and one voxel into the neighbouring columns); the update / FFD kernels read all of step 0's output.
IRS_HD ColPlan plan_column_of(const int* runs, int k, int col, int C, int ntx, int nty, int D) {
    const int tiles = ntx * nty, chain = col / tiles, tile = col - chain * tiles, tx = tile % ntx, ty = tile / ntx;
    const int* r = runs + ((long long)k * C * tiles + col) * 2;
    int nlo = 0, nhi = D;
    if (k > 0) {
        nlo = D;
        nhi = 0;
        const int* prev = runs + ((long long)(k - 1) * C + chain) * tiles * 2;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                // (a neighbour outside the grid folds onto a tile of the 3 x 3 block that is inside it: the hull is the same, and the
                // nine loads do not wait for one another)
                const int ux = plan_min(plan_max(tx + dx, 0), ntx - 1), uy = plan_min(plan_max(ty + dy, 0), nty - 1);
                const int l = prev[(uy * ntx + ux) * 2], h = prev[(uy * ntx + ux) * 2 + 1];
                if (h > l) {
                    nlo = plan_min(nlo, plan_max(l - 1, 0));
                    nhi = plan_max(nhi, plan_min(h + 1, D));
                }
            }
    }
    return plan_column(r[0], r[1], nlo, nhi);
}

// ---- the same arithmetic for any tile and reach (the data stage: adjoint_plan.hip, "sparse data stage")
constexpr int kLccTX = 32, kLccTY = 16;   // tile column of the LCC map and of the data term (stencil_kernels.hip: LMX x LMY)
constexpr int kWarpTX = 64, kWarpTY = 8;  // tile-plane of the warp (field_kernels.hip)
constexpr int kDataKernels = 4;           // read-back rows of the data stage: warp, LCC map, statistics (dense: zero), data term
enum PlanFill { kFillNext = 0, kFillAll = 1, kFillNone = 2 };  // what a list zero-fills: what the next step reads / the rest of every column / nothing
constexpr int kPlanMaxLists = 32;         // most lists a shape with per-list reaches describes (the forward steps: one per step)
// How the run ranges and the lists of one launch are formed.  List k has reach reach0 - k * reach_dec -- or, with n_reach > 0, its own
// reach[k] (the forward steps: their reaches are sums of planned widths); list 0 and the lists behind it may differ in what they
// fill and in the resident set they are cut for (the data term and the LCC map share a launch).
struct PlanShape {
    int tx, ty;
    int reach0, reach_dec;
    int fill[2];
    int G[2];
    int lmin;
    int n_reach;
    int reach[kPlanMaxLists];
};
IRS_HD int plan_reach(const PlanShape& s, int k) { return s.n_reach > 0 ? s.reach[k] : s.reach0 - k * s.reach_dec; }

// ---- sparse forward squaring steps (adjoint_plan.hip, "sparse forward steps"): d_j must be exact on W_j = mask (+) reach_j,
// reach_j = 3 S + h_j + ... + h_{n-1} (h_i: planned width of step i, floor(max|d_i|) + 1 <= h_i; S: LCC half width, SSD 0).  Forward
// step k writes d_{k+1}: its list is the hull of W_{k+1} over the forward tile's columns.
IRS_HD int plan_forward_reach(const int* h, int n, int S, int k) {
    int m = 3 * S;
    for (int i = k + 1; i < n; ++i) m += h[i];
    return m;
}
IRS_HD int plan_fill_of(const PlanShape& s, int k) { return s.fill[k > 0 ? 1 : 0]; }
IRS_HD int plan_resident_of(const PlanShape& s, int k) { return s.G[k > 0 ? 1 : 0]; }
// the voxels [a, b) of an axis of n within m of tile t of `size`
IRS_HD void plan_tile_window(int t, int size, int m, int n, int& a, int& b) {
    a = plan_max(t * size - m, 0);
    b = plan_min(t * size + size + m, n);
}
// the plan of column `col` of list k under fill rule `fill`
IRS_HD ColPlan plan_column_by(const int* runs, int k, int col, int C, int ntx, int nty, int D, int fill) {
    if (fill == kFillNext) return plan_column_of(runs, k, col, C, ntx, nty, D);
    const int* r = runs + ((long long)k * C * ntx * nty + col) * 2;
    return fill == kFillAll ? plan_column(r[0], r[1], 0, D) : plan_column(r[0], r[1], 0, 0);
}

IRS_HD int plan_pieces(int len, int L) { return len > 0 ? (len + L - 1) / L : 0; }

// piece j of np equal cuts of [lo, lo + len)
IRS_HD void plan_cut(int lo, int len, int np, int j, int& z0, int& z1) {
    z0 = lo + (int)((long long)len * j / np);
    z1 = lo + (int)((long long)len * (j + 1) / np);
}

// entry of run piece j of a column
IRS_HD PlanEntry plan_entry(const ColPlan& c, int chain, int tile, int np, int j) {
    int z0, z1;
    plan_cut(c.lo, c.hi - c.lo, np, j, z0, z1);
    return PlanEntry{chain, tile, z0, z1, 0, 0};
}
// the fill below (side 0: [f0, lo), for a column without a run range all of its fill) and above (side 1: [hi, f1)) a column's run range
IRS_HD bool plan_has_fill(const ColPlan& c, int side) { return side == 0 ? c.f0 < c.lo : c.hi < c.f1 && c.hi > c.lo; }
IRS_HD PlanEntry plan_fill_entry(const ColPlan& c, int chain, int tile, int side) {
    return side == 0 ? PlanEntry{chain, tile, c.f0, c.lo, 1, 0} : PlanEntry{chain, tile, c.hi, c.f1, 1, 0};
}

// Piece length of a step: the smallest L in [lmin, lmax] whose run pieces (pieces[L], summed over the columns) fit one resident set
// of G workgroups; lmax if none does.  The workgroups stride over the list: the fill entries behind the run pieces (a store per
// plane) go to the first workgroups once they have marched their piece.
IRS_HD int plan_pick_len(const int* pieces, int G, int lmin, int lmax) {
    for (int L = lmin; L < lmax; ++L)
        if (pieces[L] <= G) return L;
    return lmax;
}

// Most run pieces a list of `columns` columns can have: the length search stays within G unless even the longest piece does not
// fit; a forced length cuts every column at that length.  (The grid of a kernel that gives every run piece a workgroup of its own.)
IRS_HD int plan_run_bound(int columns, int D, int G, int forced_len) {
    const int lmax = plan_max(plan_min(kPlanMaxLen, D), 1);
    if (forced_len > 0) return columns * plan_pieces(D, plan_min(plan_max(forced_len, kPlanMinForced), lmax));
    return plan_max(G, columns * plan_pieces(D, lmax));
}

// entries a step's list can hold: a column gives at most ceil(D / kPlanMinForced) run pieces and two fills
IRS_HD int plan_entries_cap(int columns, int D) { return columns * ((D + kPlanMinForced - 1) / kPlanMinForced + 2); }

// ---- plan reuse (adjoint_plan.hip, "plan reuse"): a list in the workspace is a pure function of its extent table, of what the host
// passes to the launch that cuts it, and -- the adjoint -- of which chains left the radius-1 kernel.  Every list keeps a record of
// those, and the launches that would rebuild it leave at once while the record still holds.
// One entry of an extent table from a column's first and last non-zero plane (hi < 0: none): (D - lo, hi + 1), empty (0, 0).
IRS_HD void plan_extent_entry(int lo, int hi, int D, int& a, int& b) {
    a = hi < 0 ? 0 : D - lo;
    b = hi < 0 ? 0 : hi + 1;
}
enum PlanSource { kSourceGradient = 0, kSourceMask = 1 };  // the table a list was cut from: g_warped's extents or the mask's
constexpr int kPlanKeyLen = 20;
// everything the host passes in that decides list k of a launch
struct PlanKey {
    int v[kPlanKeyLen];
};
// generation of an extent table: the extent pass adds to it whenever an entry changed, so a list cut from generation g is clean
// for exactly as long as the table still says g (a consumer that was not launched for a while compares like any other)
typedef unsigned long long PlanGen;
struct PlanRecord {
    int valid;       // zeroed memory is no record
    unsigned dense;  // bit c: chain c was given full columns (chain_is_dense)
    PlanGen gen;
    PlanKey key;
};
// `lists`: how many lists the launch cuts (the adjoint's fills look at list k - 1, the dense flags at every step); `source`: PlanSource
IRS_HD PlanKey plan_key(const PlanShape& s, int k, int lists, int forced_len, int C, int ext_chains, int D, int H, int W, int source,
                        bool with_dense) {
    PlanKey key;
    const int before = k > 0 && plan_fill_of(s, k) == kFillNext ? plan_reach(s, k - 1) : -1;  // (plan_column_of reads the runs of list k - 1)
    const int v[kPlanKeyLen] = {s.tx, s.ty, plan_reach(s, k), before, plan_fill_of(s, k), plan_resident_of(s, k), s.lmin,
                                forced_len, C, ext_chains, D, H, W, source, with_dense ? 1 : 0, lists, k, 0, 0, 0};
    for (int i = 0; i < kPlanKeyLen; ++i) key.v[i] = v[i];
    return key;
}
IRS_HD bool plan_key_equal(const PlanKey& a, const PlanKey& b) {
    bool eq = true;
    for (int i = 0; i < kPlanKeyLen; ++i) eq = eq && a.v[i] == b.v[i];
    return eq;
}
// the list a record describes is, byte for byte, what a rebuild with (key, dense, gen) would write
IRS_HD bool plan_reusable(const PlanRecord& r, const PlanKey& key, unsigned dense, PlanGen gen) {
    return r.valid == 1 && r.dense == dense && r.gen == gen && plan_key_equal(r.key, key);
}
IRS_HD PlanRecord plan_record(const PlanKey& key, unsigned dense, PlanGen gen) { return PlanRecord{1, dense, gen, key}; }
// reach of the adjoint's list k of n: the gradient step k produces is zero further than n - k from the support of g_warped, which
// itself lies within 2 S of the mask (S: LCC half width, SSD 0)
IRS_HD int plan_adjoint_reach0(int n, int S, int source) { return source == kSourceMask ? 2 * S + n : n; }

// workgroup id -> list position: runs of `run` consecutive entries (x-neighbouring tiles of one z band) stay on one XCD, as
// common.h: xcd_swizzle_runs does for whole grids -- here for any count: the tail that fills no group of 8 runs keeps its order.
IRS_HD int plan_swizzle(int id, int count, int run) {
    if (run <= 1) return id;
    const int group = 8 * run;
    if (id >= count / group * group) return id;
    const int g = id / group, w = id - g * group;
    return g * group + (w & 7) * run + (w >> 3);
}

}  // namespace irs
