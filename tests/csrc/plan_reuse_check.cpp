// CPU check of plan reuse (ir_sgmcmc_amd/csrc/adjoint_plan.h: plan_key, plan_reusable, plan_record, plan_extent_entry and the splitting
// arithmetic the device kernels of adjoint_plan.hip run).  A small model of the device sequence -- extent pass with compare-and-store
// and a generation, runs stage, lists stage, one record per list -- on random masks in small ragged volumes with random widths,
// dense flags, piece lengths and resident sets, for the three kinds of list (the adjoint's: fills for the next step, dense flags;
// the forward steps': one reach per list; the data stage's: two fill rules):
//   a. a zeroed record is invalid, whatever key it is asked about;
//   b. changing any single key field, any dense flag, or any table entry (an entry inside the window of a list among them) makes
//      the predicate say "rebuild";
//   c. whenever the predicate says "reuse" -- nothing changed, or the mask changed strictly between a column's first and last
//      voxel -- the list rebuilt from scratch equals the kept one entry for entry, with its count and its run ranges;
//   d. the mask-sourced run range of every tile column of every adjoint step contains the gradient-sourced one, for a gradient
//      supported anywhere inside mask (+) 2 S.
// Prints "violations 0" and exits 0 when all hold.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../ir_sgmcmc_amd/csrc/adjoint_plan.h"

using namespace irs;

static unsigned rng_state = 2463534242u;
static unsigned rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

static long long violations = 0, reuses = 0, rebuilds = 0;
#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            if (violations < 20) {          \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);        \
                printf("\n");               \
            }                               \
            ++violations;                   \
        }                                   \
    } while (0)

struct Dims {
    int D, H, W;
};
constexpr int IRS_CHECK_CHAINS = 8;  // dense flags looked at (include/irsgmcmc.h: IRS_MAX_CHAINS)

static void random_mask(const Dims& d, std::vector<char>& m) {
    m.assign((size_t)d.D * d.H * d.W, 0);
    const int boxes = rnd_in(0, 3);
    for (int b = 0; b < boxes; ++b) {
        const int z0 = rnd_in(0, d.D - 1), y0 = rnd_in(0, d.H - 1), x0 = rnd_in(0, d.W - 1);
        const int z1 = plan_min(d.D, z0 + rnd_in(1, 9)), y1 = plan_min(d.H, y0 + rnd_in(1, 7)), x1 = plan_min(d.W, x0 + rnd_in(1, 14));
        for (int z = z0; z < z1; ++z)
            for (int y = y0; y < y1; ++y)
                for (int x = x0; x < x1; ++x) m[((size_t)z * d.H + y) * d.W + x] = 1;
    }
}

// the extent pass: the final entry of every column compared with the table, stored when it differs; the generation advances if any did
struct Table {
    std::vector<int> ext;
    PlanGen gen = 0;
};
static void extent_pass(const std::vector<char>& m, const Dims& d, Table& t) {
    if (t.ext.empty()) t.ext.assign((size_t)d.H * d.W * 2, 0);  // (the zeroed workspace: every column empty)
    bool changed = false;
    for (int y = 0; y < d.H; ++y)
        for (int x = 0; x < d.W; ++x) {
            int lo = d.D, hi = -1;
            for (int z = 0; z < d.D; ++z)
                if (m[((size_t)z * d.H + y) * d.W + x]) {
                    lo = plan_min(lo, z);
                    hi = z;
                }
            int a, b;
            plan_extent_entry(lo, hi, d.D, a, b);
            int* e = &t.ext[((size_t)y * d.W + x) * 2];
            if (e[0] != a || e[1] != b) {
                e[0] = a;
                e[1] = b;
                changed = true;
            }
        }
    if (changed) ++t.gen;
}

// one family of lists in the "workspace": what the runs stage and the lists stage leave
struct Family {
    PlanShape shape;
    int lists, forced, source, C;
    bool with_dense;
    std::vector<int> runs;                      // [lists][cols][2]
    std::vector<std::vector<PlanEntry>> entry;  // [lists]
    std::vector<int> n_run;
    std::vector<PlanRecord> rec;
};

static void runs_stage(const Family& f, int k, unsigned dense, const Table& t, const Dims& d, int ntx, int nty, std::vector<int>& runs) {
    const int tiles = ntx * nty, m = plan_reach(f.shape, k);
    for (int col = 0; col < f.C * tiles; ++col) {
        const int chain = col / tiles, tile = col - chain * tiles;
        int* out = &runs[((size_t)k * f.C * tiles + col) * 2];
        if (dense >> chain & 1u) {
            out[0] = 0;
            out[1] = d.D;
            continue;
        }
        int x0, x1, y0, y1, lo = d.D, hi = 0;
        plan_tile_window(tile % ntx, f.shape.tx, m, d.W, x0, x1);
        plan_tile_window(tile / ntx, f.shape.ty, m, d.H, y0, y1);
        for (int y = y0; y < y1; ++y)
            for (int x = x0; x < x1; ++x) {
                int l, h;
                plan_widen(t.ext[((size_t)y * d.W + x) * 2], t.ext[((size_t)y * d.W + x) * 2 + 1], m, d.D, l, h);
                if (h > l) {
                    lo = plan_min(lo, l);
                    hi = plan_max(hi, h);
                }
            }
        out[0] = hi > lo ? lo : 0;
        out[1] = hi > lo ? hi : 0;
    }
}

static void lists_stage(const Family& f, int k, const std::vector<int>& runs, const Dims& d, int ntx, int nty, std::vector<PlanEntry>& list, int& n_run) {
    const int tiles = ntx * nty, cols = f.C * tiles;
    const int lmax = plan_max(plan_min(kPlanMaxLen, d.D), 1), lmin = plan_min(f.shape.lmin, lmax);
    std::vector<int> pieces(kPlanMaxLen + 1, 0);
    std::vector<ColPlan> cps((size_t)cols);
    int maxlen = 0;
    for (int col = 0; col < cols; ++col) {
        cps[(size_t)col] = plan_column_by(runs.data(), k, col, f.C, ntx, nty, d.D, plan_fill_of(f.shape, k));
        const int len = cps[(size_t)col].hi - cps[(size_t)col].lo;
        if (len > 0) {
            for (int L = lmin; L <= lmax; ++L) pieces[L] += plan_pieces(len, L);
            maxlen = plan_max(maxlen, len);
        }
    }
    const int L = f.forced > 0 ? plan_min(plan_max(f.forced, kPlanMinForced), lmax) : plan_pick_len(pieces.data(), plan_resident_of(f.shape, k), lmin, lmax);
    const int levels = plan_pieces(maxlen, L);
    list.clear();
    n_run = 0;
    for (int j = 0; j < levels + 2; ++j)
        for (int col = 0; col < cols; ++col) {
            const ColPlan& cp = cps[(size_t)col];
            const int np = plan_pieces(cp.hi - cp.lo, L);
            if (j < levels ? j < np : plan_has_fill(cp, j - levels)) {
                list.push_back(j < levels ? plan_entry(cp, col / tiles, col % tiles, np, j) : plan_fill_entry(cp, col / tiles, col % tiles, j - levels));
                n_run += j < levels;
            }
        }
}

static PlanKey key_of(const Family& f, int k, int ext_chains, const Dims& d) {
    return plan_key(f.shape, k, f.lists, f.forced, f.C, ext_chains, d.D, d.H, d.W, f.source, f.with_dense);
}

// one transition's two launches over a family: every list whose record holds is left alone, the others are cut again.  -> lists kept
static int plan_launches(Family& f, unsigned dense, const Table& t, const Dims& d, bool reuse) {
    const int ntx = (d.W + f.shape.tx - 1) / f.shape.tx, nty = (d.H + f.shape.ty - 1) / f.shape.ty;
    if (f.runs.empty()) {
        f.runs.assign((size_t)f.lists * f.C * ntx * nty * 2, 0);
        f.entry.assign((size_t)f.lists, {});
        f.n_run.assign((size_t)f.lists, 0);
        PlanRecord zero;
        memset(&zero, 0, sizeof(zero));
        f.rec.assign((size_t)f.lists, zero);
    }
    std::vector<char> keep((size_t)f.lists);
    for (int k = 0; k < f.lists; ++k) keep[(size_t)k] = reuse && plan_reusable(f.rec[(size_t)k], key_of(f, k, 1, d), dense, t.gen);
    for (int k = 0; k < f.lists; ++k)  // the runs stage of all lists, then the lists stage (the adjoint's fills read the runs of list k - 1)
        if (!keep[(size_t)k]) runs_stage(f, k, dense, t, d, ntx, nty, f.runs);
    int kept = 0;
    for (int k = 0; k < f.lists; ++k) {
        if (keep[(size_t)k]) {
            ++kept;
            continue;
        }
        lists_stage(f, k, f.runs, d, ntx, nty, f.entry[(size_t)k], f.n_run[(size_t)k]);
        f.rec[(size_t)k] = plan_record(key_of(f, k, 1, d), dense, t.gen);
    }
    reuses += kept;
    rebuilds += f.lists - kept;
    return kept;
}

static bool same_lists(const Family& a, const Family& b) {
    if (a.runs != b.runs || a.n_run != b.n_run) return false;
    for (size_t k = 0; k < a.entry.size(); ++k) {
        if (a.entry[k].size() != b.entry[k].size()) return false;
        for (size_t i = 0; i < a.entry[k].size(); ++i)
            if (memcmp(&a.entry[k][i], &b.entry[k][i], sizeof(PlanEntry)) != 0) return false;
    }
    return true;
}

static Family make_family(int kind, int n, int S, int C) {
    Family f{};
    f.C = C;
    f.forced = rnd_in(0, 2) == 0 ? rnd_in(1, 20) : 0;
    const int G = rnd_in(1, 80);
    if (kind == 0) {  // the adjoint's lists from the mask's table
        f.lists = n;
        f.source = kSourceMask;
        f.with_dense = true;
        f.shape = PlanShape{kPlanTX, kPlanTY, plan_adjoint_reach0(n, S, kSourceMask), 1, {kFillNext, kFillNext}, {G, G}, kPlanMinLen};
    } else if (kind == 1) {  // the forward steps'
        int h[kPlanMaxLists];
        for (int i = 0; i < n; ++i) h[i] = rnd_in(1, 3);
        f.lists = n;
        f.source = kSourceMask;
        f.shape = PlanShape{kWarpTX, kWarpTY, 0, 0, {kFillNone, kFillNone}, {G, G}, kPlanMinLen, n, {}};
        for (int k = 0; k < n; ++k) f.shape.reach[k] = plan_forward_reach(h, n, S, k);
    } else {  // the data term's and the LCC map's
        f.lists = 2;
        f.source = kSourceMask;
        f.shape = PlanShape{kLccTX, kLccTY, 2 * S, S, {kFillAll, kFillNone}, {G, rnd_in(1, 80)}, kPlanMinLen};
    }
    return f;
}

// the family as a rebuild from nothing would leave it
static Family from_scratch(const Family& f, unsigned dense, const Table& t, const Dims& d) {
    Family g = f;
    g.runs.clear();
    plan_launches(g, dense, t, d, false);
    return g;
}

static void check_key_fields(const Family& f, const Dims& d, unsigned dense, PlanGen gen, int id) {
    for (int k = 0; k < f.lists; ++k) {
        const PlanKey key = key_of(f, k, 1, d);
        const PlanRecord& r = f.rec[(size_t)k];
        CHECK(plan_reusable(r, key, dense, gen), "case %d list %d: an unchanged list must be reusable", id, k);
        PlanRecord zero;
        memset(&zero, 0, sizeof(zero));
        PlanKey zero_key;
        memset(&zero_key, 0, sizeof(zero_key));
        CHECK(!plan_reusable(zero, key, dense, gen) && !plan_reusable(zero, zero_key, 0u, 0), "case %d list %d: a zeroed record is valid", id, k);  // a.
        // b. one field of what the host passes in
        Family g = f;
        g.runs.clear();
        auto differs = [&](const char* what) {
            CHECK(!plan_reusable(r, key_of(g, k, 1, d), dense, gen), "case %d list %d: a change of %s is not seen", id, k, what);
            g = f;
            g.runs.clear();
        };
        g.shape.tx *= 2, differs("the tile's width");
        g.shape.ty *= 2, differs("the tile's height");
        if (g.shape.n_reach > 0) g.shape.reach[k] += 1; else g.shape.reach0 += 1;
        differs("the reach");
        g.shape.fill[k > 0 ? 1 : 0] = (g.shape.fill[k > 0 ? 1 : 0] + 1) % 3, differs("the fill rule");
        g.shape.G[k > 0 ? 1 : 0] += 1, differs("the resident set");
        g.shape.lmin += 1, differs("the shortest piece");
        g.forced += 1, differs("the forced piece length");
        g.C += 1, differs("the chains");
        g.source = 1 - g.source, differs("the table it is cut from");
        g.with_dense = !g.with_dense, differs("whether bounds are looked at");
        g.lists += 1, differs("the number of lists");
        CHECK(!plan_reusable(r, key_of(f, k, 2, d), dense, gen), "case %d list %d: a change of the table's chains is not seen", id, k);
        const Dims d1{d.D + 1, d.H, d.W}, d2{d.D, d.H + 1, d.W}, d3{d.D, d.H, d.W + 1};
        CHECK(!plan_reusable(r, key_of(f, k, 1, d1), dense, gen) && !plan_reusable(r, key_of(f, k, 1, d2), dense, gen) &&
                  !plan_reusable(r, key_of(f, k, 1, d3), dense, gen), "case %d list %d: a change of the dims is not seen", id, k);
        if (k > 0 && f.shape.n_reach == 0) {  // (a list with fills for the next step also depends on that step's reach)
            g.shape.reach_dec += 1;
            differs("the reach of the list before it");
        }
        for (int c = 0; c < IRS_CHECK_CHAINS; ++c) CHECK(!plan_reusable(r, key, dense ^ (1u << c), gen), "case %d list %d: dense flag %d", id, k, c);
        CHECK(!plan_reusable(r, key, dense, gen + 1), "case %d list %d: a changed table is not seen", id, k);
    }
}

// the mask dilated by r voxels (Chebyshev), clipped to the volume: one pass per axis
static std::vector<char> dilate(const std::vector<char>& m, const Dims& d, int r) {
    const int n[3] = {d.D, d.H, d.W};
    const size_t stride[3] = {(size_t)d.H * d.W, (size_t)d.W, 1};
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

static void run_case(const Dims& d, int id) {
    const int S = rnd_in(0, 2), n = rnd_in(1, 6), C = rnd_in(1, 2);
    std::vector<char> mask;
    random_mask(d, mask);
    Table t;
    extent_pass(mask, d, t);
    for (int kind = 0; kind < 3; ++kind) {
        Family f = make_family(kind, n, S, C);
        unsigned dense = kind == 0 && rnd_in(0, 3) == 0 ? (unsigned)rnd_in(1, (1 << C) - 1) : 0u;
        CHECK(plan_launches(f, dense, t, d, true) == 0, "case %d kind %d: a list kept before it was ever cut", id, kind);
        check_key_fields(f, d, dense, t.gen, id);
        // c. nothing changed
        CHECK(plan_launches(f, dense, t, d, true) == f.lists, "case %d kind %d: an unchanged transition cut lists again", id, kind);
        CHECK(same_lists(f, from_scratch(f, dense, t, d)), "case %d kind %d: kept lists differ from rebuilt ones", id, kind);
        // c. the mask changes strictly inside a column: the table, and with it every list, stays
        std::vector<char> m2 = mask;
        bool flipped = false;
        for (int y = 0; y < d.H && !flipped; ++y)
            for (int x = 0; x < d.W && !flipped; ++x) {
                const int a = t.ext[((size_t)y * d.W + x) * 2], b = t.ext[((size_t)y * d.W + x) * 2 + 1];
                if (b - (d.D - a) >= 3) {
                    m2[((size_t)(d.D - a + 1) * d.H + y) * d.W + x] = 0;
                    flipped = true;
                }
            }
        Table t2 = t;
        extent_pass(m2, d, t2);
        CHECK(t2.gen == t.gen && t2.ext == t.ext, "case %d: an interior voxel changed the table", id);
        CHECK(plan_launches(f, dense, t2, d, true) == f.lists, "case %d kind %d: an interior change cut lists again", id, kind);
        CHECK(same_lists(f, from_scratch(f, dense, t2, d)), "case %d kind %d: kept lists differ from rebuilt ones (interior change)", id, kind);
        // b. a table entry changes (a voxel on top of a column, or the first voxel of an empty one): every list says "rebuild"
        const int y = rnd_in(0, d.H - 1), x = rnd_in(0, d.W - 1), hi = t.ext[((size_t)y * d.W + x) * 2 + 1];
        if (hi < d.D) m2[((size_t)hi * d.H + y) * d.W + x] = 1;
        else m2[((size_t)(d.D - 1) * d.H + y) * d.W + x] = 0;
        extent_pass(m2, d, t2);
        CHECK(t2.gen != t.gen, "case %d: a changed table entry is not seen", id);
        for (int k = 0; k < f.lists; ++k)
            CHECK(!plan_reusable(f.rec[(size_t)k], key_of(f, k, 1, d), dense, t2.gen), "case %d kind %d list %d: reuse over a changed table", id, kind, k);
        CHECK(plan_launches(f, dense, t2, d, true) == 0, "case %d kind %d: a list kept over a changed table", id, kind);
        CHECK(same_lists(f, from_scratch(f, dense, t2, d)), "case %d kind %d: rebuilt lists differ from those cut from nothing", id, kind);
        if (kind == 0) {  // a chain leaves the radius-1 kernel, and returns
            const unsigned flip = dense ^ (1u << rnd_in(0, C - 1));
            CHECK(plan_launches(f, flip, t2, d, true) == 0, "case %d: a list kept over a dense flip", id);
            CHECK(same_lists(f, from_scratch(f, flip, t2, d)), "case %d: lists after a dense flip", id);
            CHECK(plan_launches(f, dense, t2, d, true) == 0, "case %d: a list kept over the flip back", id);
            CHECK(same_lists(f, from_scratch(f, dense, t2, d)), "case %d: lists after the flip back", id);
        }
        if (kind == 1 && n > 1) {  // one planned width moves: exactly the lists whose reach moved are cut again
            Family g = f;
            const int j = rnd_in(1, n - 1);
            for (int k = 0; k < j; ++k) g.shape.reach[k] += 1;  // (h_j one wider: the reaches of the lists in front of it)
            CHECK(plan_launches(g, dense, t2, d, true) == n - j, "case %d: lists kept after width %d moved", id, j);
            CHECK(same_lists(g, from_scratch(g, dense, t2, d)), "case %d: lists after a width moved", id);
        }
        if (kind == 2) {  // the forced piece length changes
            Family g = f;
            g.forced = f.forced > 0 ? f.forced + 4 : 12;
            CHECK(plan_launches(g, dense, t2, d, true) == 0, "case %d: a list kept over another piece length", id);
            CHECK(same_lists(g, from_scratch(g, dense, t2, d)), "case %d: lists after the piece length changed", id);
        }
    }
    // d. the adjoint's run ranges from the mask's table contain those from the extents of any gradient inside mask (+) 2 S
    const std::vector<char> support = dilate(mask, d, 2 * S);
    std::vector<char> grad(support.size(), 0);
    const int keep_one_in = rnd_in(1, 4);
    for (size_t i = 0; i < grad.size(); ++i) grad[i] = support[i] && rnd_in(1, keep_one_in) == 1;
    Table tg;
    extent_pass(grad, d, tg);
    Family fm = make_family(0, n, S, C), fg = fm;
    fg.source = kSourceGradient;
    fg.shape.reach0 = plan_adjoint_reach0(n, S, kSourceGradient);
    plan_launches(fm, 0u, t, d, false);
    plan_launches(fg, 0u, tg, d, false);
    CHECK(fm.runs.size() == fg.runs.size(), "case %d: run range tables", id);
    for (size_t i = 0; i + 1 < fm.runs.size() && i + 1 < fg.runs.size(); i += 2)
        if (fg.runs[i + 1] > fg.runs[i])
            CHECK(fm.runs[i + 1] > fm.runs[i] && fm.runs[i] <= fg.runs[i] && fm.runs[i + 1] >= fg.runs[i + 1],
                  "case %d column %d: mask-sourced [%d, %d) does not contain gradient-sourced [%d, %d)", id, (int)(i / 2), fm.runs[i], fm.runs[i + 1],
                  fg.runs[i], fg.runs[i + 1]);
}

int main() {
    const Dims dims[] = {{24, 20, 70}, {40, 20, 70}, {72, 24, 40}, {7, 16, 32}, {66, 17, 65}, {3, 5, 6}};
    int id = 0;
    for (const Dims& d : dims)
        for (int rep = 0; rep < 12; ++rep) run_case(d, id++);
    printf("cases %d lists rebuilt %lld reused %lld violations %lld\n", id, rebuilds, reuses, violations);
    return violations ? 1 : 0;
}
