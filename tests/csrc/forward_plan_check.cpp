// CPU check of the sparse forward steps' regions and lists (ir_sgmcmc_amd/csrc/adjoint_plan.h: plan_forward_reach and the splitting
// arithmetic the device kernels of adjoint_plan.hip run, with the forward tile and one reach per list).  Random masks on small ragged
// volumes, random widths h_i in {1, 2, 3}, S in {0, 1, 2}, one or two chains with their own masks -> extents -> run ranges -> piece
// lists, in the kernels' order.  With W_j = mask (+) (3 S + h_j + ... + h_{n-1}) (Chebyshev dilation, j = 1 .. n), for every j:
//   a. every voxel of W_j lies in exactly one run piece of list j - 1, and the list has no fills;
//   b. W_{j+1} (+) h_j is inside W_j (forward step j finds its taps exact);
//   c. mask (+) (2 S + h_j + ... + h_{n-1}) is inside W_j (the adjoint's sources and the corners of their own term);
//   d. the last list covers the warp's hull at reach 3 S;
//   e. no piece leaves the volume or is longer than the chosen length;
//   f. the list fits its allocation (plan_entries_cap) and the grid of its kernel (plan_run_bound), and the resident set whenever a
//      length below the cap does.
// Prints "violations 0" and exits 0 when all hold.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../ir_sgmcmc_amd/csrc/adjoint_plan.h"

using namespace irs;

static unsigned rng_state = 88172645u;
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
    int D, H, W, kind, S, n, C, forced;
};

static void make_mask(int D, int H, int W, int kind, std::vector<char>& m) {
    m.assign((size_t)D * H * W, 0);
    auto at = [&](int z, int y, int x) -> char& { return m[((size_t)z * H + y) * W + x]; };
    if (kind == 1) {
        for (auto& v : m) v = 1;
    } else if (kind == 2) {  // a single corner voxel
        at(rnd_in(0, 1) ? D - 1 : 0, rnd_in(0, 1) ? H - 1 : 0, rnd_in(0, 1) ? W - 1 : 0) = 1;
    } else if (kind == 3) {  // a ball
        const double cz = (D - 1) / 2.0 + rnd_in(-3, 3), cy = (H - 1) / 2.0, cx = (W - 1) / 2.0 + rnd_in(-5, 5);
        const double r = 0.3 * plan_min(D, plan_min(H, W));
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if ((z - cz) * (z - cz) + (y - cy) * (y - cy) + (x - cx) * (x - cx) < r * r) at(z, y, x) = 1;
    } else if (kind >= 4) {  // a few random boxes
        for (int b = 0; b < kind - 2; ++b) {
            const int z0 = rnd_in(0, D - 1), y0 = rnd_in(0, H - 1), x0 = rnd_in(0, W - 1);
            const int z1 = plan_min(D, z0 + rnd_in(1, 5)), y1 = plan_min(H, y0 + rnd_in(1, 6)), x1 = plan_min(W, x0 + rnd_in(1, 12));
            for (int z = z0; z < z1; ++z)
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) at(z, y, x) = 1;
        }
    }  // kind 0: empty
}

// the mask dilated by r voxels (Chebyshev), clipped to the volume: one pass per axis
static std::vector<char> dilate(const std::vector<char>& m, int D, int H, int W, int r) {
    const int n[3] = {D, H, W};
    const size_t stride[3] = {(size_t)H * W, (size_t)W, 1};
    std::vector<char> cur = m;
    for (int a = 0; a < 3 && r > 0; ++a) {
        std::vector<char> out(cur.size(), 0);
        for (size_t i = 0; i < cur.size(); ++i) {
            if (!cur[i]) continue;
            const int p = (int)(i / stride[a] % (size_t)n[a]);
            for (int q = plan_max(p - r, 0); q <= plan_min(p + r, n[a] - 1); ++q) out[i + (size_t)(q - p) * stride[a]] = 1;
        }
        cur.swap(out);
    }
    return cur;
}
static bool inside(const std::vector<char>& a, const std::vector<char>& b) {
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i] && !b[i]) return false;
    return true;
}

// run ranges as plan_runs_kernel computes them: [list][chain tiles][2], one extent table per chain
static std::vector<int> run_ranges(const std::vector<std::vector<int>>& ext, const PlanShape& sh, int lists, int C, int D, int H, int W, int ntx,
                                   int nty) {
    const int tiles = ntx * nty;
    std::vector<int> runs((size_t)lists * C * tiles * 2, 0);
    for (int k = 0; k < lists; ++k)
        for (int col = 0; col < C * tiles; ++col) {
            const int chain = col / tiles, tile = col - chain * tiles, m = plan_reach(sh, k);
            const std::vector<int>& e = ext[ext.size() == 1 ? 0 : (size_t)chain];
            int x0, x1, y0, y1, lo = D, hi = 0;
            plan_tile_window(tile % ntx, sh.tx, m, W, x0, x1);
            plan_tile_window(tile / ntx, sh.ty, m, H, y0, y1);
            for (int y = y0; y < y1; ++y)
                for (int x = x0; x < x1; ++x) {
                    int l, h;
                    plan_widen(e[((size_t)y * W + x) * 2], e[((size_t)y * W + x) * 2 + 1], m, D, l, h);
                    if (h > l) {
                        lo = plan_min(lo, l);
                        hi = plan_max(hi, h);
                    }
                }
            runs[((size_t)k * C * tiles + col) * 2] = hi > lo ? lo : 0;
            runs[((size_t)k * C * tiles + col) * 2 + 1] = hi > lo ? hi : 0;
        }
    return runs;
}

static void run_case(const Case& cs, int id) {
    const int D = cs.D, H = cs.H, W = cs.W, S = cs.S, n = cs.n, C = cs.C;
    // per-chain masks (two chains: the second has another kind of mask) and their extent tables as mask_extent_kernel leaves them
    std::vector<std::vector<char>> mask((size_t)C);
    std::vector<std::vector<int>> ext((size_t)C, std::vector<int>((size_t)H * W * 2, 0));
    for (int c = 0; c < C; ++c) {
        make_mask(D, H, W, c == 0 ? cs.kind : (cs.kind + 3) % 7, mask[(size_t)c]);
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (mask[(size_t)c][((size_t)z * H + y) * W + x]) {
                        int* e = &ext[(size_t)c][((size_t)y * W + x) * 2];
                        e[0] = plan_max(e[0], D - z);
                        e[1] = plan_max(e[1], z + 1);
                    }
    }
    int h[kPlanMaxLists];
    for (int i = 0; i < n; ++i) h[i] = rnd_in(1, 3);
    const int ntx = (W + kWarpTX - 1) / kWarpTX, nty = (H + kWarpTY - 1) / kWarpTY, tiles = ntx * nty, cols = C * tiles;
    const int G = rnd_in(1, 80);
    PlanShape sh{kWarpTX, kWarpTY, 0, 0, {kFillNone, kFillNone}, {G, G}, kPlanMinLen, n, {}};
    for (int k = 0; k < n; ++k) sh.reach[k] = plan_forward_reach(h, n, S, k);
    CHECK(sh.reach[n - 1] == 3 * S, "case %d: the last list's reach", id);
    const std::vector<int> runs = run_ranges(ext, sh, n, C, D, H, W, ntx, nty);
    const int cap = plan_entries_cap(cols, D);
    const int lmax = plan_max(plan_min(kPlanMaxLen, D), 1), lmin = plan_min(sh.lmin, lmax);
    // ---- the regions: b. c.
    for (int c = 0; c < C; ++c)
        for (int j = 1; j <= n; ++j) {
            int tail = 0;  // h_j + ... + h_{n-1}
            for (int i = j; i < n; ++i) tail += h[i];
            CHECK(plan_reach(sh, j - 1) == 3 * S + tail, "case %d: reach of list %d", id, j - 1);
            const std::vector<char> Wj = dilate(mask[(size_t)c], D, H, W, 3 * S + tail);
            if (j < n) CHECK(inside(dilate(dilate(mask[(size_t)c], D, H, W, 3 * S + tail - h[j]), D, H, W, h[j]), Wj), "case %d chain %d: W_%d (+) h_%d leaves W_%d", id, c, j + 1, j, j);
            CHECK(inside(dilate(mask[(size_t)c], D, H, W, 2 * S + tail), Wj), "case %d chain %d: the adjoint's sources leave W_%d", id, c, j);
        }
    // ---- the lists as plan_lists_kernel builds them: a. e. f.
    for (int k = 0; k < n; ++k) {
        std::vector<int> pieces(kPlanMaxLen + 1, 0);
        int maxlen = 0;
        for (int col = 0; col < cols; ++col) {
            const ColPlan cp = plan_column_by(runs.data(), k, col, C, ntx, nty, D, plan_fill_of(sh, k));
            const int len = cp.hi - cp.lo;
            CHECK(cp.f0 == cp.lo && cp.hi == cp.f1 && cp.lo >= 0 && cp.hi <= D, "case %d list %d col %d: a fill range", id, k, col);
            if (len > 0) {
                for (int L = lmin; L <= lmax; ++L) pieces[L] += plan_pieces(len, L);
                maxlen = plan_max(maxlen, len);
            }
        }
        const int L = cs.forced > 0 ? plan_min(plan_max(cs.forced, kPlanMinForced), lmax) : plan_pick_len(pieces.data(), plan_resident_of(sh, k), lmin, lmax);
        const int levels = plan_pieces(maxlen, L);
        std::vector<PlanEntry> list;
        int n_run = 0;
        for (int j = 0; j < levels + 2; ++j)
            for (int col = 0; col < cols; ++col) {
                const ColPlan cp = plan_column_by(runs.data(), k, col, C, ntx, nty, D, plan_fill_of(sh, k));
                const int np = plan_pieces(cp.hi - cp.lo, L);
                if (j < levels ? j < np : plan_has_fill(cp, j - levels)) {
                    list.push_back(j < levels ? plan_entry(cp, col / tiles, col % tiles, np, j) : plan_fill_entry(cp, col / tiles, col % tiles, j - levels));
                    n_run += j < levels;
                }
            }
        CHECK((int)list.size() <= cap, "case %d list %d: %d entries, cap %d", id, k, (int)list.size(), cap);
        CHECK(n_run == (int)list.size(), "case %d list %d: fills in a forward list", id, k);
        CHECK(n_run <= plan_run_bound(cols, D, G, cs.forced), "case %d list %d: %d run pieces, grid %d", id, k, n_run, plan_run_bound(cols, D, G, cs.forced));
        if (cs.forced <= 0 && L < lmax) CHECK(n_run <= G, "case %d list %d: %d run pieces, G %d", id, k, n_run, G);
        std::vector<char> wr((size_t)cols * D, 0);
        for (const PlanEntry& e : list) {
            const bool ok = 0 <= e.z0 && e.z0 < e.z1 && e.z1 <= D && e.tile >= 0 && e.tile < tiles && e.chain >= 0 && e.chain < C;
            CHECK(ok && !e.fill && e.z1 - e.z0 <= L, "case %d list %d entry chain %d tile %d [%d, %d) L %d", id, k, e.chain, e.tile, e.z0, e.z1, L);
            if (!ok) continue;
            for (int z = e.z0; z < e.z1; ++z) {
                char& w = wr[((size_t)e.chain * tiles + e.tile) * D + z];
                CHECK(w == 0, "case %d list %d chain %d tile %d plane %d listed twice", id, k, e.chain, e.tile, z);
                w = 1;
            }
        }
        for (int c = 0; c < C; ++c) {
            const std::vector<char> Wj = dilate(mask[(size_t)c], D, H, W, plan_reach(sh, k));  // W_{k+1}
            for (int z = 0; z < D; ++z)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x)
                        if (Wj[((size_t)z * H + y) * W + x]) {
                            const int col = c * tiles + (y / kWarpTY) * ntx + x / kWarpTX;
                            CHECK(wr[(size_t)col * D + z] == 1, "case %d list %d chain %d voxel (%d,%d,%d) of W_%d not marched", id, k, c, z, y, x, k + 1);
                        }
        }
        // d. the warp's hull (its own launch of plan_runs_kernel at reach 3 S) is inside the last list's pieces
        if (k == n - 1) {
            const PlanShape warp{kWarpTX, kWarpTY, 3 * S, 0, {kFillNone, kFillNone}, {1, 1}, kPlanMinLen};
            const std::vector<int> hull = run_ranges(ext, warp, 1, C, D, H, W, ntx, nty);
            for (int col = 0; col < cols; ++col)
                for (int z = hull[(size_t)col * 2]; z < hull[(size_t)col * 2 + 1]; ++z)
                    CHECK(wr[(size_t)col * D + z] == 1, "case %d column %d plane %d of the warp's hull not in the last list", id, col, z);
        }
    }
}

int main() {
    const int dims[][3] = {{24, 20, 70}, {40, 20, 70}, {72, 24, 40}, {7, 16, 32}, {66, 17, 65}, {3, 5, 6}};
    int id = 0;
    for (const auto& d : dims)
        for (int kind = 0; kind <= 6; ++kind)  // 0 empty, 1 full, 2 a single corner voxel, 3 a ball, 4 .. 6 random boxes
            for (int rep = 0; rep < 3; ++rep) {
                const Case cs{d[0], d[1], d[2], kind, rnd_in(0, 2), rnd_in(1, 6), 1 + rep % 2, rep == 2 ? rnd_in(1, 20) : 0};
                run_case(cs, id++);
            }
    printf("cases %d violations %lld\n", id, violations);
    return violations ? 1 : 0;
}
