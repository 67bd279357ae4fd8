// CPU check of the sparse data stage's splitting arithmetic (ir_sgmcmc_amd/csrc/adjoint_plan.h, the code the device kernels of
// adjoint_plan.hip run with a tile and a reach passed in): random masks on small ragged volumes -> extents -> run ranges -> piece
// lists, in the kernels' order, for the 32 x 16 tile of the LCC map / data term and the 64 x 8 tile of the warp.  Then:
//   a. every voxel within the list's reach (Chebyshev) of the mask lies in exactly one run piece;
//   b. with the fill rule of the data term, every other voxel lies in exactly one fill entry; with the map's rule there are no fills;
//   c. no entry leaves the volume, run pieces are 1 .. L planes long, the list fits its allocation;
//   d. the run pieces fit the grid their kernel is launched with (plan_run_bound), and the resident set whenever a length below the
//      cap does;
//   e. a tile-plane test against the run range (the warp) keeps every voxel within reach.
// Prints "violations 0" and exits 0 when all hold.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../ir_sgmcmc_amd/csrc/adjoint_plan.h"

using namespace irs;

static unsigned rng_state = 2463534242u;
static unsigned rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

static long long violations = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (violations < 20) {        \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);      \
                printf("\n");             \
            }                             \
            ++violations;                 \
        }                                 \
    } while (0)

struct Case {
    int D, H, W, kind, s, forced;
};

static void make_mask(const Case& cs, std::vector<char>& m) {
    const int D = cs.D, H = cs.H, W = cs.W;
    m.assign((size_t)D * H * W, 0);
    auto at = [&](int z, int y, int x) -> char& { return m[((size_t)z * H + y) * W + x]; };
    if (cs.kind == 1) {
        for (auto& v : m) v = 1;
    } else if (cs.kind == 2) {
        at(rnd_in(0, 1) ? D - 1 : 0, rnd_in(0, 1) ? H - 1 : 0, rnd_in(0, 1) ? W - 1 : 0) = 1;
    } else if (cs.kind == 3) {  // a ball
        const double cz = (D - 1) / 2.0 + rnd_in(-3, 3), cy = (H - 1) / 2.0, cx = (W - 1) / 2.0 + rnd_in(-5, 5);
        const double r = 0.35 * plan_min(D, plan_min(H, W));
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if ((z - cz) * (z - cz) + (y - cy) * (y - cy) + (x - cx) * (x - cx) < r * r) at(z, y, x) = 1;
    } else if (cs.kind >= 4) {  // a few boxes, mirrored along z: two blobs in the same columns
        for (int b = 0; b < cs.kind; ++b) {
            const int z0 = rnd_in(0, D - 1), y0 = rnd_in(0, H - 1), x0 = rnd_in(0, W - 1);
            const int z1 = plan_min(D, z0 + rnd_in(1, 6)), y1 = plan_min(H, y0 + rnd_in(1, 9)), x1 = plan_min(W, x0 + rnd_in(1, 20));
            for (int z = z0; z < z1; ++z)
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) at(z, y, x) = at(D - 1 - z, y, x) = 1;
        }
    }  // kind 0: empty
}

// the mask dilated by m voxels (Chebyshev), clipped to the volume
static std::vector<char> dilate(const std::vector<char>& m, int D, int H, int W, int r) {
    std::vector<char> out(m.size(), 0);
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                if (!m[((size_t)z * H + y) * W + x]) continue;
                for (int zz = plan_max(z - r, 0); zz <= plan_min(z + r, D - 1); ++zz)
                    for (int yy = plan_max(y - r, 0); yy <= plan_min(y + r, H - 1); ++yy)
                        for (int xx = plan_max(x - r, 0); xx <= plan_min(x + r, W - 1); ++xx) out[((size_t)zz * H + yy) * W + xx] = 1;
            }
    return out;
}

// run ranges as plan_runs_kernel computes them: [list][column][2]
static std::vector<int> run_ranges(const std::vector<int>& ext, const PlanShape& sh, int lists, int D, int H, int W, int ntx, int nty) {
    std::vector<int> runs((size_t)lists * ntx * nty * 2, 0);
    for (int k = 0; k < lists; ++k)
        for (int col = 0; col < ntx * nty; ++col) {
            const int m = plan_reach(sh, k);
            int x0, x1, y0, y1, lo = D, hi = 0;
            plan_tile_window(col % ntx, sh.tx, m, W, x0, x1);
            plan_tile_window(col / ntx, sh.ty, m, H, y0, y1);
            for (int y = y0; y < y1; ++y)
                for (int x = x0; x < x1; ++x) {
                    int l, h;
                    plan_widen(ext[((size_t)y * W + x) * 2], ext[((size_t)y * W + x) * 2 + 1], m, D, l, h);
                    if (h > l) {
                        lo = plan_min(lo, l);
                        hi = plan_max(hi, h);
                    }
                }
            runs[((size_t)k * ntx * nty + col) * 2] = hi > lo ? lo : 0;
            runs[((size_t)k * ntx * nty + col) * 2 + 1] = hi > lo ? hi : 0;
        }
    return runs;
}

static void run_case(const Case& cs, int id) {
    const int D = cs.D, H = cs.H, W = cs.W, s = cs.s;
    std::vector<char> mask;
    make_mask(cs, mask);
    // extent table as mask_extent_kernel leaves it
    std::vector<int> ext((size_t)H * W * 2, 0);
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (mask[((size_t)z * H + y) * W + x]) {
                    int* e = &ext[((size_t)y * W + x) * 2];
                    e[0] = plan_max(e[0], D - z);
                    e[1] = plan_max(e[1], z + 1);
                }
    // ---- the lists of the data term (list 0: reach 2 s, fills the rest) and of the map (list 1: reach s, no fills)
    {
        const int ntx = (W + kLccTX - 1) / kLccTX, nty = (H + kLccTY - 1) / kLccTY, cols = ntx * nty;
        const int G[2] = {rnd_in(1, 60), rnd_in(1, 60)};
        const PlanShape sh{kLccTX, kLccTY, 2 * s, s, {kFillAll, kFillNone}, {G[0], G[1]}, kPlanMinLen};
        const std::vector<int> runs = run_ranges(ext, sh, 2, D, H, W, ntx, nty);
        const int cap = plan_entries_cap(cols, D);
        const int lmax = plan_max(plan_min(kPlanMaxLen, D), 1), lmin = plan_min(sh.lmin, lmax);
        for (int k = 0; k < 2; ++k) {
            // the list as plan_lists_kernel builds it
            std::vector<int> pieces(kPlanMaxLen + 1, 0);
            int maxlen = 0;
            for (int col = 0; col < cols; ++col) {
                const ColPlan cp = plan_column_by(runs.data(), k, col, 1, ntx, nty, D, plan_fill_of(sh, k));
                const int len = cp.hi - cp.lo;
                CHECK(cp.f0 <= cp.lo && cp.hi <= cp.f1 && cp.f0 >= 0 && cp.f1 <= D, "case %d list %d col %d", id, k, col);
                if (len > 0) {
                    for (int L = lmin; L <= lmax; ++L) pieces[L] += plan_pieces(len, L);
                    maxlen = plan_max(maxlen, len);
                }
            }
            const int L = cs.forced > 0 ? plan_min(plan_max(cs.forced, kPlanMinForced), lmax)
                                        : plan_pick_len(pieces.data(), plan_resident_of(sh, k), lmin, lmax);
            const int levels = plan_pieces(maxlen, L);
            std::vector<PlanEntry> list;
            int n_run = 0;
            for (int j = 0; j < levels + 2; ++j)
                for (int col = 0; col < cols; ++col) {
                    const ColPlan cp = plan_column_by(runs.data(), k, col, 1, ntx, nty, D, plan_fill_of(sh, k));
                    const int np = plan_pieces(cp.hi - cp.lo, L);
                    if (j < levels ? j < np : plan_has_fill(cp, j - levels)) {
                        list.push_back(j < levels ? plan_entry(cp, 0, col, np, j) : plan_fill_entry(cp, 0, col, j - levels));
                        n_run += j < levels;
                    }
                }
            // c. d.
            CHECK((int)list.size() <= cap, "case %d list %d: %d entries, cap %d", id, k, (int)list.size(), cap);
            CHECK(n_run <= plan_run_bound(cols, D, plan_resident_of(sh, k), cs.forced), "case %d list %d: %d run pieces, grid %d", id, k, n_run,
                  plan_run_bound(cols, D, plan_resident_of(sh, k), cs.forced));
            if (cs.forced <= 0 && L < lmax) CHECK(n_run <= plan_resident_of(sh, k), "case %d list %d: %d run pieces, G %d", id, k, n_run, plan_resident_of(sh, k));
            std::vector<char> wr((size_t)cols * D, 0);  // per (column, plane): 1 marched, 2 filled
            for (const PlanEntry& e : list) {
                CHECK(0 <= e.z0 && e.z0 < e.z1 && e.z1 <= D && e.tile >= 0 && e.tile < cols && (e.fill || e.z1 - e.z0 <= L),
                      "case %d list %d entry tile %d [%d, %d)", id, k, e.tile, e.z0, e.z1);
                if (!(0 <= e.z0 && e.z1 <= D && e.tile >= 0 && e.tile < cols)) continue;
                for (int z = e.z0; z < e.z1; ++z) {
                    CHECK(wr[(size_t)e.tile * D + z] == 0, "case %d list %d tile %d plane %d listed twice", id, k, e.tile, z);
                    wr[(size_t)e.tile * D + z] = e.fill ? 2 : 1;
                }
            }
            // a. b.
            const std::vector<char> reach = dilate(mask, D, H, W, plan_reach(sh, k));
            for (int z = 0; z < D; ++z)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        const int col = (y / kLccTY) * ntx + x / kLccTX, w = wr[(size_t)col * D + z];
                        if (reach[((size_t)z * H + y) * W + x]) CHECK(w == 1, "case %d list %d voxel (%d,%d,%d) within reach, not marched", id, k, z, y, x);
                        else if (plan_fill_of(sh, k) == kFillAll) CHECK(w == 1 || w == 2, "case %d list %d voxel (%d,%d,%d) neither marched nor filled", id, k, z, y, x);
                        if (plan_fill_of(sh, k) == kFillNone) CHECK(w != 2, "case %d list %d: a fill in the map's list", id, k);
                    }
        }
    }
    // ---- e. the hull of the warp: 64 x 8 tile-planes at reach 3 s (SSD: 0)
    for (int reach_w : {3 * s, 0}) {
        const int ntx = (W + kWarpTX - 1) / kWarpTX, nty = (H + kWarpTY - 1) / kWarpTY;
        const PlanShape sh{kWarpTX, kWarpTY, reach_w, 0, {kFillNone, kFillNone}, {1, 1}, kPlanMinLen};
        const std::vector<int> hull = run_ranges(ext, sh, 1, D, H, W, ntx, nty);
        const std::vector<char> reach = dilate(mask, D, H, W, reach_w);
        for (int col = 0; col < ntx * nty; ++col) CHECK(0 <= hull[col * 2] && hull[col * 2] <= hull[col * 2 + 1] && hull[col * 2 + 1] <= D, "case %d hull of tile %d", id, col);
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (reach[((size_t)z * H + y) * W + x]) {
                        const int col = (y / kWarpTY) * ntx + x / kWarpTX;
                        CHECK(z >= hull[col * 2] && z < hull[col * 2 + 1], "case %d voxel (%d,%d,%d) within %d of the mask, outside the hull", id, z, y, x, reach_w);
                    }
    }
}

int main() {
    const int dims[][3] = {{24, 20, 70}, {40, 20, 70}, {72, 24, 40}, {7, 16, 32}, {130, 17, 65}, {3, 5, 6}};
    int id = 0;
    for (const auto& d : dims)
        for (int kind = 0; kind <= 6; ++kind)
            for (int rep = 0; rep < 3; ++rep) {
                const Case cs{d[0], d[1], d[2], kind, rnd_in(1, 2), rep == 2 ? rnd_in(1, 20) : 0};
                run_case(cs, id++);
            }
    printf("cases %d violations %lld\n", id, violations);
    return violations ? 1 : 0;
}
