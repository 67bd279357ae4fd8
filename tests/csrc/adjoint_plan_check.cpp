// CPU check of the sparse adjoint plan's splitting arithmetic (ir_sgmcmc_amd/csrc/adjoint_plan.h, the code the device kernels of
// adjoint_plan.hip run): random supports of g_warped on small ragged volumes -> extents -> run ranges -> piece lists, in the kernels'
// order, then the properties the adjoint relies on:
//   a. no plane of a tile column is written twice in a step (run pieces and fills are disjoint);
//   b. every voxel within m = n - k voxels (Chebyshev) of the support lies in a run piece of step k;
//   c. every plane a piece of step k - 1 reads -- its own range and one plane either side, in its tile column and the 8 around it --
//      was written (marched or zero-filled) by step k;
//   d. step 0 writes every plane of every column;
//   e. the list fits its allocation, run pieces are 1 .. L planes long, and fit the resident set whenever a length below the cap does;
//   f. the workgroup -> entry remap is a bijection.
// Prints "violations 0" and exits 0 when all hold.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../ir_sgmcmc_amd/csrc/adjoint_plan.h"

using namespace irs;

static unsigned rng_state = 12345u;
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
    int D, H, W, n, G, forced, kind;
};

static void run_case(const Case& cs, int id) {
    const int D = cs.D, H = cs.H, W = cs.W, n = cs.n;
    const int ntx = (W + kPlanTX - 1) / kPlanTX, nty = (H + kPlanTY - 1) / kPlanTY, cols = ntx * nty;
    std::vector<char> supp((size_t)D * H * W, 0);
    auto at = [&](int z, int y, int x) -> char& { return supp[((size_t)z * H + y) * W + x]; };
    if (cs.kind == 1) {
        for (auto& s : supp) s = 1;
    } else if (cs.kind == 2) {
        at(rnd_in(0, 1) ? D - 1 : 0, rnd_in(0, 1) ? H - 1 : 0, rnd_in(0, 1) ? W - 1 : 0) = 1;
    } else if (cs.kind >= 3) {  // a few boxes (two of them stacked along z in the same columns)
        for (int b = 0; b < cs.kind; ++b) {
            const int z0 = rnd_in(0, D - 1), y0 = rnd_in(0, H - 1), x0 = rnd_in(0, W - 1);
            const int z1 = plan_min(D, z0 + rnd_in(1, 6)), y1 = plan_min(H, y0 + rnd_in(1, 9)), x1 = plan_min(W, x0 + rnd_in(1, 20));
            for (int z = z0; z < z1; ++z)
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) at(z, y, x) = at(D - 1 - z, y, x) = 1;
        }
    }  // kind 0: empty
    // extent table as grad_extent_kernel leaves it
    std::vector<int> ext((size_t)H * W * 2, 0);
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (at(z, y, x)) {
                    int* e = &ext[((size_t)y * W + x) * 2];
                    e[0] = plan_max(e[0], D - z);
                    e[1] = plan_max(e[1], z + 1);
                }
    // run ranges as plan_runs_kernel computes them
    std::vector<int> runs((size_t)n * cols * 2, 0);
    for (int k = 0; k < n; ++k)
        for (int col = 0; col < cols; ++col) {
            const int tx = col % ntx, ty = col / ntx, m = n - k;
            int lo = D, hi = 0;
            for (int y = plan_max(ty * kPlanTY - m, 0); y < plan_min(ty * kPlanTY + kPlanTY + m, H); ++y)
                for (int x = plan_max(tx * kPlanTX - m, 0); x < plan_min(tx * kPlanTX + kPlanTX + m, W); ++x) {
                    int l, h;
                    plan_widen(ext[((size_t)y * W + x) * 2], ext[((size_t)y * W + x) * 2 + 1], m, D, l, h);
                    if (h > l) {
                        lo = plan_min(lo, l);
                        hi = plan_max(hi, h);
                    }
                }
            runs[((size_t)k * cols + col) * 2] = hi > lo ? lo : 0;
            runs[((size_t)k * cols + col) * 2 + 1] = hi > lo ? hi : 0;
        }
    const int cap = plan_entries_cap(cols, D);
    const int lmax = plan_max(plan_min(kPlanMaxLen, D), 1), lmin = plan_min(kPlanMinLen, lmax);
    std::vector<char> reach = supp;                        // support dilated n - k times, k = n - 1 first
    std::vector<char> written_next;                        // [col][z] of step k + 1 (0: not written)
    std::vector<std::vector<PlanEntry>> lists(n);
    std::vector<std::vector<char>> written(n);
    for (int k = n - 1; k >= 0; --k) {
        // lists as plan_lists_kernel builds them
        std::vector<int> pieces(kPlanMaxLen + 1, 0);
        int maxlen = 0;
        for (int col = 0; col < cols; ++col) {
            const ColPlan cp = plan_column_of(runs.data(), k, col, 1, ntx, nty, D);
            const int len = cp.hi - cp.lo;
            CHECK(cp.f0 <= cp.lo && cp.hi <= cp.f1 && cp.f0 >= 0 && cp.f1 <= D, "case %d step %d col %d", id, k, col);
            if (len > 0) {
                for (int L = lmin; L <= lmax; ++L) pieces[L] += plan_pieces(len, L);
                maxlen = plan_max(maxlen, len);
            }
        }
        const int L = cs.forced > 0 ? plan_min(plan_max(cs.forced, kPlanMinForced), lmax) : plan_pick_len(pieces.data(), cs.G, lmin, lmax);
        const int levels = plan_pieces(maxlen, L);
        std::vector<PlanEntry>& list = lists[k];
        int n_run = 0;
        for (int j = 0; j < levels + 2; ++j)
            for (int col = 0; col < cols; ++col) {
                const ColPlan cp = plan_column_of(runs.data(), k, col, 1, ntx, nty, D);
                const int np = plan_pieces(cp.hi - cp.lo, L);
                if (j < levels ? j < np : plan_has_fill(cp, j - levels)) {
                    list.push_back(j < levels ? plan_entry(cp, 0, col, np, j) : plan_fill_entry(cp, 0, col, j - levels));
                    n_run += j < levels;
                }
            }
        CHECK((int)list.size() <= cap, "case %d step %d: %d entries, cap %d", id, k, (int)list.size(), cap);
        if (cs.forced <= 0 && L < lmax) CHECK(n_run <= cs.G, "case %d step %d: %d run pieces, G %d, L %d", id, k, n_run, cs.G, L);
        // a. what the step writes
        std::vector<char>& wr = written[k];
        wr.assign((size_t)cols * D, 0);
        for (const PlanEntry& e : list) {
            CHECK(0 <= e.z0 && e.z0 < e.z1 && e.z1 <= D && (e.fill || e.z1 - e.z0 <= L), "case %d step %d entry [%d, %d)", id, k, e.z0, e.z1);
            for (int z = e.z0; z < e.z1; ++z) {
                CHECK(wr[(size_t)e.tile * D + z] == 0, "case %d step %d tile %d plane %d written twice", id, k, e.tile, z);
                wr[(size_t)e.tile * D + z] = e.fill ? 2 : 1;
            }
        }
        // b. the gradient's reach lies in run pieces
        {
            std::vector<char> next(reach.size(), 0);
            for (int z = 0; z < D; ++z)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        if (!reach[((size_t)z * H + y) * W + x]) continue;
                        for (int dz = -1; dz <= 1; ++dz)
                            for (int dy = -1; dy <= 1; ++dy)
                                for (int dx = -1; dx <= 1; ++dx) {
                                    const int zz = z + dz, yy = y + dy, xx = x + dx;
                                    if (zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W) next[((size_t)zz * H + yy) * W + xx] = 1;
                                }
                    }
            reach.swap(next);
            for (int z = 0; z < D; ++z)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x)
                        if (reach[((size_t)z * H + y) * W + x]) {
                            const int col = (y / kPlanTY) * ntx + x / kPlanTX;
                            CHECK(wr[(size_t)col * D + z] == 1, "case %d step %d voxel (%d,%d,%d) not marched", id, k, z, y, x);
                        }
        }
        // d. step 0 writes everything
        if (k == 0)
            for (size_t i = 0; i < wr.size(); ++i) CHECK(wr[i] != 0, "case %d step 0: plane %d of column %d unwritten", id, (int)(i % D), (int)(i / D));
        // f. the remap
        for (int run : {0, 1, ntx, 3}) {
            std::vector<char> seen(list.size(), 0);
            for (int i = 0; i < (int)list.size(); ++i) {
                const int p = plan_swizzle(i, (int)list.size(), run);
                CHECK(p >= 0 && p < (int)list.size() && !seen[p], "case %d step %d: remap of %d (run %d)", id, k, i, run);
                if (p >= 0 && p < (int)list.size()) seen[p] = 1;
            }
        }
    }
    // c. what step k - 1 reads, step k wrote
    for (int k = 1; k < n; ++k)
        for (const PlanEntry& e : lists[k - 1]) {
            if (e.fill) continue;
            const int tx = e.tile % ntx, ty = e.tile / ntx;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int ux = tx + dx, uy = ty + dy;
                    if (ux < 0 || ux >= ntx || uy < 0 || uy >= nty) continue;
                    for (int z = plan_max(e.z0 - 1, 0); z < plan_min(e.z1 + 1, D); ++z)
                        CHECK(written[k][(size_t)(uy * ntx + ux) * D + z] != 0, "case %d: step %d reads plane %d of tile %d, unwritten by step %d", id,
                              k - 1, z, uy * ntx + ux, k);
                }
        }
}

int main() {
    const int dims[][3] = {{24, 20, 70}, {40, 9, 33}, {72, 24, 40}, {7, 8, 32}, {130, 17, 65}, {3, 5, 6}};
    int id = 0;
    for (const auto& d : dims)
        for (int kind = 0; kind <= 5; ++kind)
            for (int rep = 0; rep < 3; ++rep) {
                const Case cs{d[0], d[1], d[2], rnd_in(1, 12), rep == 0 ? 1024 : rnd_in(1, 40), rep == 2 ? rnd_in(1, 20) : 0, kind};
                run_case(cs, id++);
            }
    printf("cases %d violations %lld\n", id, violations);
    return violations ? 1 : 0;
}
