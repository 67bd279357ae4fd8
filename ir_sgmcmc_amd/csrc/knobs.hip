// The tuning / test switches (common.h: Knobs): one table of names and scopes behind both the IRS_* environment variables and
// irs_option_set; the launch log; the count of live contexts that the layout switches are checked against.
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ctx.h"

namespace irs {

// Scope of a switch.  CTX: copied into a context at creation and read from there (`irs_option_set(ctx, ...)` changes that copy,
// `irs_option_set(NULL, ...)` the default of contexts created later -- and the stateless operators).  GLOBAL: the launchers read
// the process-wide value at every launch; naming a context for it is an error (it used to be accepted and ignored).  LAYOUT:
// GLOBAL, and the value also sizes the per-block partial sums a context lays out when it is created (irs_ctx::nll_blocks ...):
// changing it while a context is alive would make launches disagree with that layout, so it is refused then.
enum { KN_CTX = 0, KN_GLOBAL = 1, KN_LAYOUT = 2 };

// Every switch, once.  The environment variable of a row is IRS_ + its name in upper case.
struct Switch {
    const char* name;
    int Knobs::*field;
    int scope;
};
static const Switch kSwitches[] = {
    {"predict_variants", &Knobs::predict_variants, KN_CTX},
    {"run_ahead", &Knobs::run_ahead, KN_CTX},
    {"fuse_warp_bwd", &Knobs::fuse_warp_bwd, KN_CTX},
    {"energy_in_update", &Knobs::energy_in_update, KN_CTX},
    {"fuse_noise", &Knobs::fuse_noise, KN_CTX},
    {"recover", &Knobs::recover, KN_CTX},
    {"chain_overlap", &Knobs::chain_overlap, KN_CTX},
    {"data_batch", &Knobs::data_batch, KN_CTX},
    {"slab_split", &Knobs::slab_split, KN_CTX},
    {"slab_buffers", &Knobs::slab_buffers, KN_CTX},
    {"slab_exact", &Knobs::slab_exact, KN_CTX},
    {"slab_force_h", &Knobs::slab_force_h, KN_CTX},
    {"fwd_rows1", &Knobs::fwd_rows1, KN_GLOBAL},
    {"coarse_box", &Knobs::coarse_box, KN_GLOBAL},
    {"lds_from", &Knobs::lds_from, KN_GLOBAL},
    {"fwd_pf", &Knobs::fwd_pf, KN_GLOBAL},
    {"tile_box", &Knobs::tile_box, KN_GLOBAL},
    {"fwd_r2_rows1", &Knobs::fwd_r2_rows1, KN_GLOBAL},
    {"sobolev_tile", &Knobs::sobolev_tile, KN_GLOBAL},
    {"march_seg", &Knobs::march_seg, KN_GLOBAL},
    {"march_seg_fwd", &Knobs::march_seg_fwd, KN_GLOBAL},
    {"swz_run", &Knobs::swz_run, KN_GLOBAL},
    {"sobolev_seg", &Knobs::sobolev_seg, KN_GLOBAL},
    {"ps_rows", &Knobs::ps_rows, KN_GLOBAL},
    {"launch_log", &Knobs::launch_log, KN_GLOBAL},
    {"similarity_aggregate", &Knobs::similarity_aggregate, KN_GLOBAL},
    {"seg_fit", &Knobs::seg_fit, KN_LAYOUT},
    {"seg_min_blocks", &Knobs::seg_min_blocks, KN_LAYOUT},
    {"seg_min_len", &Knobs::seg_min_len, KN_LAYOUT},
    {"lcc_seg", &Knobs::lcc_seg, KN_LAYOUT},
    {"stats_seg", &Knobs::stats_seg, KN_LAYOUT},
    {"update_seg", &Knobs::update_seg, KN_LAYOUT},
};

static Knobs knobs_from_env() {
    Knobs k;
    for (const Switch& s : kSwitches) {
        char var[64] = "IRS_";
        size_t n = strlen(var);
        for (const char* p = s.name; *p && n + 1 < sizeof(var); ++p) var[n++] = (char)toupper((unsigned char)*p);
        var[n] = 0;
        const char* v = getenv(var);
        if (!v || !*v) continue;
        // IRS_SOBOLEV_TILE also goes by "big" / "small"
        const bool letter = s.field == &Knobs::sobolev_tile && (v[0] == 'b' || v[0] == 's');
        k.*(s.field) = letter ? (v[0] == 'b' ? 2 : 1) : atoi(v);
    }
    return k;
}

Knobs& global_knobs() {
    static Knobs k = knobs_from_env();  // the only place the library reads IRS_* tuning variables, once per process
    return k;
}

static int g_live_contexts = 0;  // contexts alive in this process (a context is not thread-safe, and neither is this count)
void context_born() { ++g_live_contexts; }
void context_gone() { --g_live_contexts; }

int knob_set(Knobs& k, const char* name, int value, bool on_context) {
    if (!name) return fail("irs_option_set: null name");
    for (const Switch& s : kSwitches)
        if (!strcmp(s.name, name)) {
            if (on_context && s.scope != KN_CTX)
                return fail("irs_option_set: '%s' is a process-wide switch (the launchers read it at every launch): set it with ctx == NULL", name);
            if (!on_context && s.scope == KN_LAYOUT && g_live_contexts > 0 && k.*(s.field) != value)
                return fail("irs_option_set: '%s' sizes the partial-sum layout of a context at creation; %d context(s) are alive -- set it before irs_create", name, g_live_contexts);
            k.*(s.field) = value;
            return 0;
        }
    return fail("irs_option_set: unknown option '%s'", name);
}

void log_launch(const char* kernel, int tile_x, int tile_y, int64_t blocks, int threads, int seg_len, int run_in, int planes_out,
                int chains, int64_t resident) {
    if (!global_knobs().launch_log) return;
    static uint64_t seen[256];
    static int n_seen = 0;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
    for (const char* p = kernel; *p; ++p) mix((uint64_t)*p);
    mix((uint64_t)blocks); mix((uint64_t)threads); mix((uint64_t)seg_len); mix((uint64_t)planes_out); mix((uint64_t)chains);
    for (int i = 0; i < n_seen; ++i)
        if (seen[i] == h) return;
    if (n_seen < 256) seen[n_seen++] = h;
    const int steps = (seg_len < planes_out ? seg_len : planes_out) + run_in;
    const double rounds = resident > 0 ? (double)blocks / (double)resident : 0.0;
    fprintf(stderr, "[irs launch] {\"kernel\": \"%s\", \"tile\": [%d, %d], \"workgroups\": %lld, \"threads\": %d, \"seg_len\": %d, \"run_in\": %d, "
                    "\"planes_out\": %d, \"chains\": %d, \"plane_steps\": %d, \"resident\": %lld, \"rounds\": %.3f, \"run_in_overhead\": %.3f}\n",
            kernel, tile_x, tile_y, (long long)blocks, threads, seg_len, run_in, planes_out, chains, steps, (long long)resident, rounds,
            (double)steps / (double)(steps - run_in > 0 ? steps - run_in : 1));
}

}  // namespace irs

extern "C" int irs_option_set(irs_ctx* ctx, const char* name, int value) {
    return irs::knob_set(ctx ? ctx->kn : irs::global_knobs(), name, value, ctx != nullptr);
}
