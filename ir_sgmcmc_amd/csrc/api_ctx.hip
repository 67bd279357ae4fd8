// C ABI (include/irsgmcmc.h), the context: its workspace, state and scalars, and the launch sequence of one SG-MCMC transition
// with the recovery from failed variant predictions.  No exceptions / aborts cross this boundary; errors come back as codes +
// irs_last_error().  The stateless operators are in api_ops.hip, the z-slab decomposition of a context in slab.hip.
#include <math.h>
#include <string.h>

#include <new>

#include "adjoint_plan.h"
#include "api_checks.h"
#include "comm.h"

using namespace irs;

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

static bool is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    return cap != hipStreamCaptureStatusNone;
}

// ================================================================================================
// context
// ================================================================================================

int irs::create_ctx(const irs_config* cfg, const SlabInfo* sl, irs_ctx** out) {
    if (!cfg || !out) return fail("irs_create: null argument");
    const int D = cfg->dims[0], H = cfg->dims[1], W = cfg->dims[2], C = cfg->no_chains;
    if (!dims_ok(C, D, H, W) || !chain_count_ok(C)) return fail("irs_create: bad dims / chains (C <= %d)", IRS_MAX_CHAINS);
    if (cfg->no_steps < 1 || cfg->no_steps > 30) return fail("irs_create: no_steps out of range");
    if (cfg->sobolev_s < 0 || cfg->sobolev_s > IRS_MAX_HALF_WIDTH) return fail("irs_create: sobolev_s out of range");
    if (cfg->data_loss != IRS_DATA_GMM_LCC && cfg->data_loss != IRS_DATA_SSD && cfg->data_loss != IRS_DATA_LNCC &&
        cfg->data_loss != IRS_DATA_MI && cfg->data_loss != IRS_DATA_NGF)
        return fail("irs_create: unknown data loss");
    if (cfg->data_loss == IRS_DATA_GMM_LCC) {
        if (!lcc_ok(cfg->lcc_s, D, H, W)) return fail("irs_create: LCC half width must be 1 or 2");
        if (cfg->gmm_components < 1 || cfg->gmm_components > IRS_MAX_COMPONENTS) return fail("irs_create: 1..%d mixture components", IRS_MAX_COMPONENTS);
    } else if (cfg->data_loss == IRS_DATA_LNCC) {
        // (the window radius travels in lcc_s; weight and eps through irs_lncc_set)
        if (cfg->lcc_s < 1 || cfg->lcc_s > IRS_MAX_HALF_WIDTH) return fail("irs_create: LNCC radius = %d, 1..%d", cfg->lcc_s, IRS_MAX_HALF_WIDTH);
        if (D < 2 * cfg->lcc_s + 1 || H < 2 * cfg->lcc_s + 1 || W < 2 * cfg->lcc_s + 1)
            return fail("irs_create: LNCC radius %d needs every dim >= %d", cfg->lcc_s, 2 * cfg->lcc_s + 1);
        if (cfg->virtual_decimation != 0) return fail("irs_create: the LNCC data term takes no virtual decimation");
    } else if (cfg->data_loss == IRS_DATA_MI) {
        // (the bins travel in lcc_s; weight and the two intensity ranges through irs_mi_set)
        if (cfg->lcc_s < IRS_MI_MIN_BINS || cfg->lcc_s > IRS_MI_MAX_BINS)
            return fail("irs_create: MI bins = %d, %d..%d", cfg->lcc_s, IRS_MI_MIN_BINS, IRS_MI_MAX_BINS);
        if (cfg->virtual_decimation != 0) return fail("irs_create: the MI data term takes no virtual decimation");
    } else if (cfg->data_loss == IRS_DATA_NGF) {
        // (lcc_s is not read; weight and the two edge parameters travel through irs_ngf_set)
        if (cfg->virtual_decimation != 0) return fail("irs_create: the NGF data term takes no virtual decimation");
    } else if (!(cfg->ssd_sigma > 0.0f)) return fail("irs_create: ssd_sigma must be positive");
    if (cfg->reg_loss < IRS_REG_L2 || cfg->reg_loss > IRS_REG_LOGNORMAL_L2) return fail("irs_create: unknown regulariser");
    if (cfg->diff_op != IRS_DIFF_GRADIENT && cfg->diff_op != IRS_DIFF_HESSIAN)
        return fail("irs_create: unknown diff_op %d (IRS_DIFF_GRADIENT or IRS_DIFF_HESSIAN; zero the irs_config before filling it)", cfg->diff_op);
    if ((cfg->reg_loss == IRS_REG_STUDENT || cfg->reg_loss == IRS_REG_LOGNORMAL_L2) && cfg->reg_learnable)
        return fail("irs_create: RegLoss_Student / RegLoss_LogNormal_L2 have no learnable parameters");
    if (cfg->reg_loss == IRS_REG_STUDENT && !(cfg->w_reg_prior_rate > 0.0 && cfg->w_reg_prior_shape > 0.0))
        return fail("irs_create: RegLoss_Student needs a0 > 0 and b0 > 0 (w_reg_prior_shape / w_reg_prior_rate)");
    const bool any_cps = cfg->cps[0] || cfg->cps[1] || cfg->cps[2];
    if (any_cps && (cfg->cps[0] < 1 || cfg->cps[1] < 1 || cfg->cps[2] < 1 || cfg->cps[0] > 8 || cfg->cps[1] > 8 || cfg->cps[2] > 8))
        return fail("irs_create: control point spacing must be 1..8 on every axis");

    irs_ctx* c = new (std::nothrow) irs_ctx();
    if (!c) return fail("irs_create: out of host memory");
    memset((void*)c, 0, sizeof(*c));
    context_born();
    c->kn = global_knobs();
    c->sparse_adjoint = true;  // (irs_sparse_adjoint_set)
    c->sparse_data = 1;        // (irs_sparse_data_set)
    c->sparse_forward = 1;     // (irs_sparse_forward_set)
    c->sparse_plan = 1;        // (irs_sparse_plan_set)
    c->lncc_weight = 1.0f;     // (irs_lncc_set)
    c->lncc_eps = 1e-5f;
    c->mi_weight = 1.0f;       // (irs_mi_set)
    c->cfg = *cfg;
    c->C = C;
    c->vol = make_vol(D, H, W);
    if (sl && sl->on) {  // slab-local arrays: the channel / chain stride is the number of HELD planes (common.h: Vol)
        c->sl = *sl;
        c->vol.V = (int64_t)(sl->hi - sl->lo) * H * W;
    }
    c->ffd = any_cps;
    c->volv = c->ffd ? make_vol(control_points(D, cfg->cps[0]), control_points(H, cfg->cps[1]), control_points(W, cfg->cps[2]))
                     : c->vol;
    // (a velocity grid narrower than the 2 s + 1 taps of the Sobolev kernel -- an SVFFD control grid of a small volume -- is fine: every
    // smoothing kernel reads through clamped coordinates, which IS the reference's replicate padding, however often a tap folds back)
    c->sob.s = cfg->sobolev_s;
    for (int i = 0; i <= 2 * cfg->sobolev_s; ++i) c->sob.k[i] = cfg->sobolev_kernel[i];
    if (c->ffd)
        for (int a = 0; a < 3; ++a) c->spl[a] = make_spline(cfg->cps[a]);

    DevCfg& d = c->dcfg;
    d.K = cfg->data_loss == IRS_DATA_GMM_LCC ? cfg->gmm_components : 1;
    // (the statistics and scalar stages of an LNCC, MI or NGF context only count the mask: to them it is an SSD context with
    // 1 / sigma = 0)
    d.mode = cfg->data_loss == IRS_DATA_LNCC || cfg->data_loss == IRS_DATA_MI || cfg->data_loss == IRS_DATA_NGF ? IRS_DATA_SSD
                                                                                                                : cfg->data_loss;
    d.vd = cfg->virtual_decimation;
    d.C = C;
    d.gmm_lr_log_std = cfg->gmm_lr_log_std;
    d.gmm_lr_logits = cfg->gmm_lr_logits;
    d.gmm_lr_decay = cfg->gmm_lr_decay;
    d.beta1 = cfg->adam_beta1 > 0 ? cfg->adam_beta1 : 0.9f;
    d.beta2 = cfg->adam_beta2 > 0 ? cfg->adam_beta2 : 0.999f;
    d.eps = cfg->adam_eps > 0 ? cfg->adam_eps : 1e-8f;
    d.scale_prior_loc = cfg->scale_prior_loc;
    d.scale_prior_scale = cfg->scale_prior_scale;
    for (int k = 0; k < IRS_MAX_COMPONENTS; ++k) d.conc[k] = cfg->dirichlet_concentration[k];
    d.reg_loss = cfg->reg_loss;
    d.reg_learnable = cfg->reg_learnable;
    d.dof = cfg->dof;
    d.reg_lr0 = cfg->reg_lr0;
    d.reg_lr1 = cfg->reg_lr1;
    d.reg_lr_decay = cfg->reg_lr_decay;
    d.loc_prior_nu = cfg->loc_prior_nu;
    d.loc_prior_w_reg = cfg->loc_prior_w_reg;
    d.reg_scale_prior_loc = cfg->reg_scale_prior_loc;
    d.reg_scale_prior_scale = cfg->reg_scale_prior_scale;
    d.w_reg_prior_shape = cfg->w_reg_prior_shape;
    d.w_reg_prior_rate = cfg->w_reg_prior_rate;

    // ---- one slab for the whole workspace
    const size_t fieldI = (size_t)C * 3 * c->vol.V * sizeof(float);   // image-grid field
    const size_t fieldV = (size_t)C * 3 * c->volv.V * sizeof(float);  // velocity-grid field
    const size_t imageI = (size_t)C * c->vol.V * sizeof(float);
    // scratch of the three axis passes: (C 3, planes held, G1 G2) + the larger of (., H, G2) [up] and (., H, G2) after (., H W -> G2) [adjoint]
    size_t ffd_tmp = 0;
    if (c->ffd) {
        const size_t planes = (size_t)(c->vol.V / ((int64_t)H * W)), g1 = c->volv.H, g2 = c->volv.W;
        ffd_tmp = sizeof(float) * (size_t)C * 3 * planes * ((size_t)g1 * g2 + (size_t)H * g2 + (size_t)H * W);
    }
    // several chains in one (unsharded) engine: their data terms run as ONE launch (transition: `data_batch`), so the segment length
    // is the one that fits ALL chains into a resident set -- at 128^3, C = 2: 7-plane segments, 1216 workgroups of 11 plane steps in
    // one round instead of two launches of 1024 with 8 each
    c->nll_seg_C = (C > 1 && !sl && cfg->data_loss == IRS_DATA_GMM_LCC && c->kn.data_batch != 0) ? C : 1;
    const bool lncc = cfg->data_loss == IRS_DATA_LNCC;
    const bool mi = cfg->data_loss == IRS_DATA_MI;  // (its finish kernel writes the data term of a chain: one "partial" per chain)
    const bool ngf = cfg->data_loss == IRS_DATA_NGF;  // (the launch shape of the LNCC kernels at radius 1)
    c->nll_blocks = lncc  ? lncc_geometry(D, H, W, cfg->lcc_s).blocks
                    : ngf ? lncc_geometry(D, H, W, 1).blocks
                    : mi  ? 1
                          : data_bwd_blocks(cfg->data_loss, c->vol, c->nll_seg_C);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
    const size_t o_steps = take(fieldI * cfg->no_steps);
    const size_t o_tmpA = take(fieldV > ffd_tmp ? fieldV : ffd_tmp);
    const size_t o_tmpB = take(fieldV);
    const size_t o_vs = take(fieldV);
    const size_t o_gA = take(fieldI), o_gB = take(fieldI);
    // a z-slab of several ranks rotates the adjoint's gradient through THREE fields: a backward exchange round may then span three
    // squaring steps (slab.hip: plan_rounds) -- held planes only, 1 / world of the volume
    const bool third = sl && sl->on && sl->world > 1;
    const size_t o_gC = third ? take(fieldI) : 0;
    const size_t o_warped = take(imageI), o_z = take(imageI), o_sig = take(imageI), o_fhat = take(imageI), o_gM = take(imageI);
    const size_t o_dense = take(c->ffd ? fieldI : 0);
    const size_t o_lncc = take(lncc ? 3 * imageI : 0);  // the coefficient maps p, q, t of the LNCC data term
    const size_t o_ngf = take(ngf ? 3 * imageI : 0);    // the coefficient maps c_z, c_y, c_x of the NGF data term
    const size_t mi_cells = mi ? (size_t)C * cfg->lcc_s * cfg->lcc_s : 0;  // the MI data term: histograms, tables, statistics, counts
    const size_t o_mi_hist = take(mi_cells * sizeof(unsigned long long)), o_mi_table = take(mi_cells * sizeof(float));
    const size_t o_mi_stats = take(mi ? sizeof(double) * C * IRS_MI_STATS : 0);
    const size_t o_mi_ipart = take(mi ? sizeof(long long) * IRS_MI_MAX_BLOCKS * 3 : 0);
    const size_t o_stat = take(sizeof(double) * kMaxPartialBlocks * kStatVals);
    const size_t o_energy = take(sizeof(double) * kMaxPartialBlocks * IRS_MAX_CHAINS);
    const size_t o_nll = take(sizeof(double) * (size_t)c->nll_blocks * C);
    const size_t o_sums = take(sizeof(double) * (kStatVals + 2 * IRS_MAX_CHAINS));
    const size_t o_dmax = take(sizeof(unsigned) * 4 * IRS_MAX_CHAINS * 32);
    const size_t o_cmm = take(coarse_minmax_bytes(c->vol, C));
    const bool planned = !sl;  // (the slab engine marches full columns)
    const size_t o_plan = take(planned ? adjoint_plan_bytes(c->vol, C, cfg->no_steps) : 0);
    const size_t o_dplan = take(planned ? data_plan_bytes(c->vol, C) : 0);
    const size_t o_fplan = take(planned && !c->ffd ? forward_plan_bytes(c->vol, C, cfg->no_steps) : 0);
    const size_t o_state = take(sizeof(DevState));
    c->slab_bytes = off;
    // (a context is zeroed at birth and irs_destroy releases whatever exists by then: one teardown for every failure below)
    if (hipMalloc((void**)&c->slab, off) != hipSuccess) {
        irs_destroy(c);
        return fail("irs_create: hipMalloc of %zu workspace bytes failed", off);
    }
    // What nobody has written yet must hold finite values: the ghost planes of a slab, and whatever the sparse data stage leaves
    // unwritten far from the mask, which later kernels read and multiply by an exact zero (sigma_M is divided by: 1 below)
    if (hipMemset(c->slab, 0, off) != hipSuccess ||
        hipMemsetD32((hipDeviceptr_t)(c->slab + o_sig), 0x3f800000, imageI / sizeof(float)) != hipSuccess) {
        irs_destroy(c);
        return fail("irs_create: clearing the workspace failed");
    }
    c->steps = (float*)(c->slab + o_steps);
    c->tmpA = (float*)(c->slab + o_tmpA);
    c->tmpB = (float*)(c->slab + o_tmpB);
    c->vs = (float*)(c->slab + o_vs);
    c->gA = (float*)(c->slab + o_gA);
    c->gB = (float*)(c->slab + o_gB);
    c->gC = third ? (float*)(c->slab + o_gC) : nullptr;
    c->warped = (float*)(c->slab + o_warped);
    c->z = (float*)(c->slab + o_z);
    c->sigM = (float*)(c->slab + o_sig);
    c->fhat = (float*)(c->slab + o_fhat);
    c->gM = (float*)(c->slab + o_gM);
    c->dense = c->ffd ? (float*)(c->slab + o_dense) : nullptr;
    c->lncc_coef = lncc ? (float*)(c->slab + o_lncc) : nullptr;
    c->ngf_coef = ngf ? (float*)(c->slab + o_ngf) : nullptr;
    c->mi_hist = mi ? (unsigned long long*)(c->slab + o_mi_hist) : nullptr;
    c->mi_table = mi ? (float*)(c->slab + o_mi_table) : nullptr;
    c->mi_stats = mi ? (double*)(c->slab + o_mi_stats) : nullptr;
    c->mi_ipart = mi ? (long long*)(c->slab + o_mi_ipart) : nullptr;
    c->stat_partials = (double*)(c->slab + o_stat);
    c->energy_partials = (double*)(c->slab + o_energy);
    c->nll_partials = (double*)(c->slab + o_nll);
    c->stat_sum = (double*)(c->slab + o_sums);
    c->energy_sum = c->stat_sum + kStatVals;
    c->nll_sum = c->energy_sum + IRS_MAX_CHAINS;
    c->dmax = (unsigned*)(c->slab + o_dmax);
    c->cmm = (float*)(c->slab + o_cmm);
    if (planned) c->plan = adjoint_plan_views(c->slab + o_plan, c->vol, C, cfg->no_steps);
    if (planned) c->dplan = data_plan_views(c->slab + o_dplan, c->vol, C);
    if (planned && !c->ffd) c->fplan = forward_plan_views(c->slab + o_fplan, c->vol, C, cfg->no_steps);
    c->state = (DevState*)(c->slab + o_state);

    if (ensure_lin_tables(c->lin, D, H, W, nullptr)) {
        irs_destroy(c);
        return fail("irs_create: identity grid allocation failed");
    }
    // initial hyper-parameters as the reference constructors set them (model/loss.py:49-50,191-192,298-303)
    DevState init;
    memset(&init, 0, sizeof(init));
    init.K = d.K;
    init.mode = d.mode;
    init.ssd_inv_sigma = cfg->data_loss == IRS_DATA_SSD ? 1.0f / cfg->ssd_sigma : 0.0f;
    if (cfg->reg_loss == IRS_REG_L2 || cfg->reg_loss == IRS_REG_LOGNORMAL_L2) init.st.reg_param[0] = log((double)cfg->w_reg);
    // (RegLoss_LogNormal's loc / log_scale need digamma: the host wrapper sets them through irs_set_state)
    for (int ch = 0; ch < IRS_MAX_CHAINS; ++ch) init.sc.alpha[ch] = 1.0;
    hipError_t e = hipMemcpy(c->state, &init, sizeof(init), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_refresh_derived(c->state, c->dcfg, nullptr);
        e = hipDeviceSynchronize();
    }
    for (int i = 0; i < 8 && e == hipSuccess; ++i) e = hipEventCreate(&c->ev[i]);
    for (int i = 0; i < 64 && e == hipSuccess; ++i) e = hipEventCreate(&c->ev_bwd[i]);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->ra_ev[i], hipEventDisableTiming);
    if (c->C > 1 && !c->sl.on && c->kn.chain_overlap) {  // the fused engine with several chains: side stream of the per-chain stage (off by default)
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
        for (int i = 0; i < 2 * c->C && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->ev_side[i], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->hint, sizeof(unsigned) * kHintWords, hipHostMallocDefault);
    if (e == hipSuccess)
        for (int i = 0; i < kHintWords; ++i) c->hint[i] = i < kHintWords - 8 ? 0x7f800000u : 0u;  // +inf: nothing known yet, launch every variant; flags clear
    if (e != hipSuccess) {
        irs_destroy(c);
        return fail("irs_create: state initialisation failed: %s", hipGetErrorString(e));
    }
    *out = c;
    return 0;
}

int irs::check_io(const irs_ctx* c, const irs_io* io, const char* who) {
    if (!c || !io) return fail("%s: null argument", who);
    if (!io->fixed_im || !io->moving_im || !io->mask) return fail("%s: fixed_im, moving_im and mask are required", who);
    if (!broadcast_ok(io->fixed_chains, c->C) || !broadcast_ok(io->moving_chains, c->C) || !broadcast_ok(io->mask_chains, c->C))
        return fail("%s: *_chains must be 1 or no_chains", who);
    if (c->cfg.data_loss == IRS_DATA_GMM_LCC && !c->fixed_set) return fail("%s: call irs_set_fixed first", who);
    if (c->cfg.data_loss == IRS_DATA_MI && !c->mi_set)
        return fail("%s: the MI data term needs irs_mi_set(ctx, weight, f_lo, f_hi, m_lo, m_hi) first: the library does not guess intensity ranges", who);
    if (c->cfg.data_loss == IRS_DATA_NGF && !c->ngf_set)
        return fail("%s: the NGF data term needs irs_ngf_set(ctx, weight, eps_f, eps_m) first: the library does not guess an edge parameter", who);
    return 0;
}

extern "C" {

int irs_create(const irs_config* cfg, irs_ctx** out) { return irs::create_ctx(cfg, nullptr, out); }

void irs_destroy(irs_ctx* c) {
    if (!c) return;
    (void)hipDeviceSynchronize();
    if (c->sl.on) slab_release(c);
    for (int i = 0; i < 8; ++i)
        if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    for (int i = 0; i < 64; ++i)
        if (c->ev_bwd[i]) (void)hipEventDestroy(c->ev_bwd[i]);
    for (int i = 0; i < 4; ++i)
        if (c->ra_ev[i]) (void)hipEventDestroy(c->ra_ev[i]);
    for (int i = 0; i < 2 * IRS_MAX_CHAINS; ++i)
        if (c->ev_side[i]) (void)hipEventDestroy(c->ev_side[i]);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->lin.dev) (void)hipFree(c->lin.dev);
    if (c->hint) (void)hipHostFree(c->hint);
    if (c->slab) (void)hipFree(c->slab);
    delete c;
    context_gone();
}

size_t irs_workspace_bytes(const irs_ctx* c) { return c ? c->slab_bytes : 0; }

int irs_velocity_dims(const irs_ctx* c, int32_t out[3]) {
    if (!c || !out) return fail("irs_velocity_dims: null argument");
    out[0] = c->volv.D;
    out[1] = c->volv.H;
    out[2] = c->volv.W;
    return 0;
}

int irs_set_fixed(irs_ctx* c, const float* fixed_im, int fixed_chains, void* stream) {
    if (!c || !fixed_im || !broadcast_ok(fixed_chains, c->C)) return fail("irs_set_fixed: bad arguments");
    if (c->cfg.data_loss == IRS_DATA_GMM_LCC) {
        Vol w = c->vol;
        int64_t shift = 0;
        if (c->sl.on) {  // slab-local image: normalise where the 2 s input planes either side are held (or are replicate padding)
            const int ls = c->cfg.lcc_s;
            w = window(c->vol, c->sl.lo + (c->sl.lo > 0 ? 2 * ls : 0), c->sl.hi - (c->sl.hi < c->vol.D ? 2 * ls : 0));
            shift = (int64_t)c->sl.lo * c->vol.H * c->vol.W;
        }
        launch_lcc_fwd_march(nullptr, 0, fixed_im - shift, c->fhat - shift, nullptr, c->cfg.lcc_s, fixed_chains, w, (hipStream_t)stream);
        LAUNCH_CHECK();
    }
    c->fhat_chains = fixed_chains;
    c->fixed_set = true;
    return 0;
}

// A slab context whose transport has FAILED (a peer gone: csrc/ipc.hip, fail-safe timeout) cannot flush -- nothing can be re-run --
// but what the device holds is well defined: the state after the last GOOD transition (the failed one was a no-op).  Reading it
// must still work: it is what a dying run checkpoints.
static int flush_or_failed_transport(irs_ctx* c, void* stream) {
    if (!irs_flush(c, stream)) return 0;
    if (!(c->sl.on && c->comm && irs::comm_check(c->comm))) return 1;
    (void)hipStreamSynchronize((hipStream_t)stream);
    if (c->cs) (void)hipStreamSynchronize(c->cs);
    return 0;
}

int irs_get_state(irs_ctx* c, irs_state* out, void* stream) {
    if (!c || !out) return fail("irs_get_state: null argument");
    if (flush_or_failed_transport(c, stream)) return 1;  // transitions that ended as no-ops are re-run first: the state is final
    HIP_TRY(hipMemcpyAsync(out, &c->state->st, sizeof(irs_state), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

static void drop_pending(irs_ctx* c);

int irs_set_state(irs_ctx* c, const irs_state* in, void* stream) {
    if (!c || !in) return fail("irs_set_state: null argument");
    // The chain is being replaced (resume, hand-over from the VI stage): transitions of the OLD chain that were dropped by a
    // failed prediction and not re-run yet must not be re-run on the restored one.  Wait, take note of the count, forget them.
    if (is_capturing((hipStream_t)stream))
        return fail("irs_set_state: the stream is being captured -- this call waits for the stream, which a capture forbids");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (c->sl.on) irs::slab_drop_pending(c);
    else drop_pending(c);
    HIP_TRY(hipMemcpyAsync(&c->state->st, in, sizeof(irs_state), hipMemcpyHostToDevice, (hipStream_t)stream));
    launch_refresh_derived(c->state, c->dcfg, (hipStream_t)stream);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int irs_get_scalars(irs_ctx* c, irs_scalars* out, void* stream) {
    if (!c || !out) return fail("irs_get_scalars: null argument");
    if (flush_or_failed_transport(c, stream)) return 1;
    HIP_TRY(hipMemcpyAsync(out, &c->state->sc, sizeof(irs_scalars), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// ================================================================================================
// the transition
// ================================================================================================
// velocity (v + noise, smoothed) -> vs; dense velocity -> d_1..d_n; warp -> warped; residual -> z (+ sigM)
// data_on (ctx.h): > 0 the warp leaves the tile-planes outside the data plan's hull unwritten, > 1 the LCC map walks its list
// fwd_lists: the squaring steps walk the lists of c->fplan (launch_forward_plan has run on this stream)
static int forward_pass(irs_ctx* c, const irs_io* io, const float* v, bool with_noise, bool with_jitter, float* vs,
                        float* warped, float* z, float* gradm, int chains, hipStream_t st, int timed, int data_on = 0, bool fwd_lists = false) {
    const irs_config& cfg = c->cfg;
    const int C = chains;
    const uint64_t* it = &c->state->st.iteration;
    // (the finalize kernel of a transition leaves the bound scratch cleared for the next one)
    if (!c->dmax_clean) HIP_TRY(hipMemsetAsync(c->dmax, 0, sizeof(unsigned) * 4 * c->C * (cfg.no_steps + 1), st));
    c->dmax_clean = false;
    // 1. SGLD perturbation + Sobolev smoothing: one kernel that generates the noise while it stages its planes (v + noise is
    //    never materialised); the two-kernel form for the mixture initialisation (no noise) and the small SVFFD control grid
    bool have_dmax0 = false;
    const float amp = (float)sqrt(2.0 * (double)cfg.lr);
    // (a sigma FIELD -- the preconditioner of a chain started from the VI posterior -- takes the kernel's 32 x 16 tile: 99 VGPRs, two
    // workgroups per CU; only sigma together with INJECTED noise, which tests use, keeps the two-kernel form)
    if (with_noise && cfg.sobolev_s > 0 && !c->ffd && c->kn.fuse_noise && !(io->sigma && io->eps)) {
        have_dmax0 = true;
        launch_perturb_sobolev_march(v, io->sigma, io->eps, amp, vs, c->sob, C, c->volv, c->dmax, cfg.no_steps, cfg.seed, 0, it, st);
    } else if (!with_noise && c->sghmc && v == io->v && cfg.sobolev_s > 0) {
        // a transition under SGHMC (irs_sghmc_set): the noise enters with the momentum, in the update; the smoothing reads v where it lies
        have_dmax0 = !c->ffd;
        launch_sobolev_march(v, vs, c->sob, C * 3, c->volv, have_dmax0 ? c->dmax : nullptr, cfg.no_steps, st);
    } else {
        float* first = cfg.sobolev_s > 0 ? c->tmpA : vs;
        if (with_noise) launch_perturb(v, io->sigma, io->eps, amp, first, C, c->volv, cfg.seed, 0, it, st);
        else HIP_TRY(hipMemcpyAsync(first, v, (size_t)C * 3 * c->volv.V * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (cfg.sobolev_s > 0) {
            have_dmax0 = !c->ffd;
            launch_sobolev_march(c->tmpA, vs, c->sob, C * 3, c->volv, have_dmax0 ? c->dmax : nullptr, cfg.no_steps, st);
        }
    }
    // 2. dense velocity
    const float* dense = vs;
    if (c->ffd) {
        const int G[3] = {c->volv.D, c->volv.H, c->volv.W};
        ffd_up(vs, c->dense, c->tmpA, C, c->vol, G, c->spl, st);
        dense = c->dense;
    }
    // 3. scaling and squaring
    if (timed) HIP_TRY(hipEventRecord(c->ev[1], st));
    const int64_t field = (int64_t)c->C * 3 * c->vol.V;
    const Lin lin = c->lin.lin();
    if (!have_dmax0) launch_field_absmax(dense, true, cfg.no_steps, c->dmax, C, c->vol, st);  // bound of d_0
    for (int k = 0; k < cfg.no_steps; ++k) {
        const float* in = k == 0 ? dense : c->steps + (int64_t)(k - 1) * field;
        float* out = c->steps + (int64_t)k * field;
        if (fwd_lists)
            launch_exp_step_fwd_plan(in, out, k == 0, cfg.no_steps, C, c->vol, lin, c->dmax + (int64_t)(k + 1) * c->C * 4, fwd_lay(c, k), c->fplan, k,
                                     c->sparse_forward > 1 ? c->sparse_forward : 0, st);
        else
            launch_exp_step_fwd_march(in, out, k == 0, cfg.no_steps, C, c->vol, lin, c->dmax + (int64_t)k * c->C * 4,
                                      c->dmax + (int64_t)(k + 1) * c->C * 4, predicted_small(c, k), fwd_lay(c, k), st);
    }
    if (timed) HIP_TRY(hipEventRecord(c->ev[2], st));
    const float* d_last = c->steps + (int64_t)(cfg.no_steps - 1) * field;
    // 4. warp (+ jitter) and residual
    const float alpha = with_jitter ? cfg.uniform_alpha : 0.0f;
    launch_warp_fwd(io->moving_im, io->moving_chains == 1 ? 0 : c->vol.V, d_last, io->unif, alpha, warped, gradm, 1, C, c->vol, lin,
                    cfg.seed, 0, it, st, data_on > 0 ? c->dplan.hull : nullptr);
    if (cfg.data_loss == IRS_DATA_GMM_LCC && data_on > 1)
        launch_lcc_fwd_plan(c->fhat, c->fhat_chains == 1 ? 0 : c->vol.V, warped, z, c->sigM, cfg.lcc_s, C, c->vol, c->dplan, st);
    else if (cfg.data_loss == IRS_DATA_GMM_LCC)
        launch_lcc_fwd_march(c->fhat, c->fhat_chains == 1 ? 0 : c->vol.V, warped, z, c->sigM, cfg.lcc_s, C, c->vol, st);
    else if (cfg.data_loss == IRS_DATA_LNCC)  // d into z, the coefficient maps for the adjoint, weight * sum mask * d per workgroup
        launch_lncc_fwd(io->fixed_im, io->fixed_chains == 1 ? 0 : c->vol.V, warped, nullptr, 0, io->mask, io->mask_chains == 1 ? 0 : c->vol.V,
                        cfg.lcc_s, c->lncc_eps, (double)c->lncc_weight, z, c->lncc_coef, c->nll_partials, C,
                        lncc_geometry(c->vol.D, c->vol.H, c->vol.W, cfg.lcc_s), st);
    else if (cfg.data_loss == IRS_DATA_NGF)  // mask * d into z, the coefficient maps for the adjoint, weight * sum mask * d per workgroup
        launch_ngf_fwd(io->fixed_im, io->fixed_chains == 1 ? 0 : c->vol.V, warped, nullptr, 0, io->mask, io->mask_chains == 1 ? 0 : c->vol.V,
                       c->ngf_eps_f, c->ngf_eps_m, (double)c->ngf_weight, true, z, c->ngf_coef, c->nll_partials, C,
                       lncc_geometry(c->vol.D, c->vol.H, c->vol.W, 1), st);
    else if (cfg.data_loss == IRS_DATA_MI) {  // histogram -> table T and the data term of every chain (nll_blocks = 1)
        // (z is only written behind the statistics stage, by the gradient kernel: what that stage multiplies by 0 must be finite)
        if (io->residuals) HIP_TRY(hipMemsetAsync(z, 0, (size_t)C * c->vol.V * sizeof(float), st));
        HIP_TRY(launch_mi_fwd(io->fixed_im, io->fixed_chains == 1 ? 0 : c->vol.V, warped, io->mask, io->mask_chains == 1 ? 0 : c->vol.V, c->vol.V,
                              C, c->mi_bins, c->mi_hist, c->mi_table, c->mi_stats, c->mi_ipart, (double)c->mi_weight, c->nll_partials, 1, st));
    } else
        launch_residual_ssd(io->fixed_im, io->fixed_chains == 1 ? 0 : c->vol.V, warped, z, C, c->vol, st);
    LAUNCH_CHECK();
    return 0;
}

int irs_gmm_init(irs_ctx* c, const irs_io* io, const float* v_sample, int warm_up, void* stream) {
    if (check_io(c, io, "irs_gmm_init")) return 1;
    if (c->cfg.data_loss != IRS_DATA_GMM_LCC) return 0;
    hipStream_t st = (hipStream_t)stream;
    // trainer.py:529-547: one velocity sample (no Langevin noise, no jitter), batch of one
    // staged in tmpB: a velocity-grid-sized buffer the forward pass does not touch (gA is image-grid-sized, and the control
    // grid of SVFFD with cps = 1 is LARGER than the image grid)
    const size_t bytes = (size_t)3 * c->volv.V * sizeof(float);
    if (v_sample) HIP_TRY(hipMemcpyAsync(c->tmpB, v_sample, bytes, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemsetAsync(c->tmpB, 0, bytes, st));
    if (forward_pass(c, io, c->tmpB, false, false, c->vs, c->warped, c->z, nullptr, 1, st, 0)) return 1;
    launch_masked_moments(c->z, io->mask, c->stat_partials, c->vol, st);
    launch_gmm_init_from_moments(c->state, c->stat_partials, stats_blocks(c->vol), c->dcfg, st);
    launch_stats(c->cfg.virtual_decimation, c->z, io->mask, c->state, c->stat_partials, c->vol, st, c->dcfg.K);
    launch_chain_scalar(c->state, c->stat_partials, stats_blocks(c->vol), 0, 1, c->dcfg, st);  // alpha, fixed below
    for (int i = 0; i < warm_up; ++i) {
        launch_stats(0, c->z, io->mask, c->state, c->stat_partials, c->vol, st, c->dcfg.K);
        launch_chain_scalar(c->state, c->stat_partials, stats_blocks(c->vol), 0, 2, c->dcfg, st);
    }
    LAUNCH_CHECK();
    return 0;
}

// One transition, enqueued.  `no_assumptions`: launch every kernel variant (nothing about max|d_k| is assumed, the transition
// cannot end as a no-op) -- the mode of the re-runs after a failed prediction.
static int enqueue_transition(irs_ctx* c, const irs_io* io, hipStream_t st, int timed, bool no_assumptions) {

    const irs_config& cfg = c->cfg;
    const int C = c->C;
    const Vol vol = c->vol, volv = c->volv;
    const Lin lin = c->lin.lin();
    float* vs = io->curr_state ? io->curr_state : c->vs;
    float* warped = io->im_moving_warped ? io->im_moving_warped : c->warped;
    float* z = io->residuals ? io->residuals : c->z;
    const uint64_t* it = &c->state->st.iteration;
    const int saved_mode = c->kn.predict_variants;
    if (no_assumptions) c->kn.predict_variants = 0;
    struct Restore {
        irs_ctx* c;
        int mode;
        ~Restore() { c->kn.predict_variants = mode; }
    } restore{c, saved_mode};

    // Which adjoint variants this transition launches, decided NOW from the bounds the host last saw (never waited for).  The
    // any-radius LDS-scatter kernel is launched only when the bound of d_k is near 2 voxels; otherwise the (rarely selected)
    // radius-2 kernel owns everything above one voxel -- through its generic in-kernel fallback if the bound exceeds its ring
    // after all.  Below 0.4 voxel (2.5x margin) the radius-2 variant is not launched either: that one IS an assumption
    // (max|d_k| < 1, the radius-1 gather has no fallback), so it goes into the verdict the device evaluates after the forward
    // pass (scalar_kernels.h: Verdict): if it does not hold the transition is a no-op and is re-run (irs_transition below).
    bool skip_any[32], skip_r2[32];
    note_hint_trend(c);
    Verdict vd = no_verdict();
    vd.bounds = c->dmax;
    vd.n = cfg.no_steps;
    vd.C = C;
    for (int k = 0; k < cfg.no_steps && k < 32; ++k) {
        skip_any[k] = predicted_below(c, k, global_knobs().lds_from <= 2 ? 0.75f : 1.5f);
        skip_r2[k] = skip_any[k] && predicted_tiny(c, k);
        if (skip_r2[k]) vd.need_lt1 |= 1u << k;
        // ... and with the any-radius kernel left out a step must stay within the radius-2 gather's ring: its generic fallback beyond
        // it is correct, but sums in another order than the kernel a chain that launches every variant uses there -- and WHICH of the
        // two ran would depend on how old the bounds were that the host happened to see.  Part of the verdict instead: the chain is
        // the same chain, bit for bit, whatever the host guessed (tests/test_gpu_recovery_fuzz.py found the difference).
        // (lds_from 2: the any-radius kernel owns everything beyond ONE voxel when it is launched, so leaving it out assumes that)
        else if (skip_any[k]) (global_knobs().lds_from > 2 ? vd.need_lt2 : vd.need_lt1) |= 1u << k;
    }

    if (timed) HIP_TRY(hipEventRecord(c->ev[0], st));
    // fused backward warp: the forward warp also writes d(warped)/d(d_last) into gA, and the first adjoint squaring step
    // multiplies it with g_warped while staging (kernels.h: gscale)
    const bool fuse_warp_bwd = c->kn.fuse_warp_bwd != 0;
    // Sparse data stage (adjoint_plan.hip): the z-extent of the mask, found now on the device, decides which tile-planes the warp
    // computes and which pieces the LCC map and the data term march.  What stays unwritten holds
    // the zeros (sigma_M: ones) of irs_create or an earlier transition's values, and is only ever multiplied by an exact zero -- in
    // the context's own buffers: a caller who asks for the warped image or the residuals gets the dense stage.  The rule on sizes:
    // only where the full-column LCC launches use segments above the shortest piece (256^3: 19 and 26 planes).  At 128^3 they are 4
    // to 8 planes in less than one resident set: lists could only match them, and the plan's launches would be a net cost there, as
    // for the adjoint below.
    const bool lcc = cfg.data_loss == IRS_DATA_GMM_LCC;
    // LNCC: its window reads beyond the mask, and so does the stencil of NGF; MI: its histogram wants every masked voxel of the warped
    // image -- no sparse data / forward stage for any of them
    const bool mi = cfg.data_loss == IRS_DATA_MI;
    const bool ngf = cfg.data_loss == IRS_DATA_NGF;
    const bool lncc = cfg.data_loss == IRS_DATA_LNCC || mi || ngf;
    const int forced_piece = c->sparse_data > 1 ? c->sparse_data : 0;  // (tests: short pieces on small volumes)
    int data_on = 0;
    c->dplan.forced_len = forced_piece;
    if (!lncc && c->sparse_data && c->dplan.entries && !io->im_moving_warped && !io->residuals &&
        (forced_piece > 0 || plan_min(lcc_dense_seg_len(vol, C, false), lcc_dense_seg_len(vol, c->nll_seg_C, true)) > kPlanMinLen)) {
        // the data term's list needs every chain in one launch (or a single chain); the per-chain launches keep their full columns
        const bool one_launch = C == 1 || (c->kn.data_batch != 0 && !(c->side && c->kn.chain_overlap != 0));
        data_on = !lcc ? 1 : one_launch ? 3 : 2;
    }
    c->data_on = data_on;
    // Sparse forward steps (adjoint_plan.hip): d_j is only read within 3 S + h_j + ... + h_{n-1} of the mask -- by the warp, by the
    // forward steps behind it and by the adjoint, whose gradient is zero further out -- where h_i is how far step i reaches,
    // floor(max|d_i|) + 1.  The widths are PLANNED here from the bounds the host last saw, with the safety factor of a slab's ghost
    // widths, go into the verdict, and are checked on the device after the forward pass: a step that outgrew its width makes the
    // transition a no-op that is re-run without assumptions, which means dense.  Only where every width can be planned (a valid
    // hint for every step, production prediction, no re-run, no capture), the any-radius adjoint is left out for every step (it takes
    // maxima over whole fields), the data plan has formed the extent table, nobody asked for the fields themselves, and -- the rule
    // on sizes -- the dense launch uses segments above the shortest piece in its two-rows form (not at 128^3).
    const int fwd_forced = c->sparse_forward > 1 ? c->sparse_forward : 0;
    bool fwd_on = c->sparse_forward != 0 && data_on > 0 && c->fplan.entries != nullptr && !c->ffd && !io->transformation && !io->displacement &&
                  c->kn.predict_variants == 1 && !no_assumptions && !is_capturing(st) && c->hint != nullptr && cfg.no_steps <= kPlanMaxLists &&
                  (fwd_forced > 0 || exp_fwd_dense_allows_lists(vol, C));
    for (int k = 0; k < cfg.no_steps && fwd_on; ++k) {
        bool valid;
        const float m = hint_row_max(c->hint + (size_t)k * C * 4, C * 4, &valid);
        // (slab_force_h on a context without a slab: every planned width forced -- a deliberately wrong plan for the validation to catch)
        const int h = !valid ? -1 : c->kn.slab_force_h > 0 ? c->kn.slab_force_h : ghost_width_from_bound(m, true);
        fwd_on = skip_any[k] && h >= 1 && h <= 255;
        c->fwd_width[k] = h;
    }
    c->fwd_on = fwd_on;
    if (fwd_on)
        for (int k = 0; k < cfg.no_steps; ++k) vd.width[k] = (unsigned char)c->fwd_width[k];
    // the mask's extent pass and the lists of the data stage and of the forward steps: three launches, which leave at once where the
    // lists in the workspace are still what they would write (adjoint_plan.hip: plan reuse)
    if (data_on > 0)
        launch_front_plans(io->mask, io->mask_chains, c->dplan, lcc ? cfg.lcc_s : 0, lcc, fwd_on ? &c->fplan : nullptr, c->fwd_width, cfg.no_steps,
                           exp_fwd_plan_resident(), fwd_forced, C, vol, c->sparse_plan, st);
    if (forward_pass(c, io, io->v, !c->sghmc, cfg.uniform_alpha > 0.0f, vs, warped, z, fuse_warp_bwd ? c->gA : nullptr, C, st, timed, data_on, fwd_on)) return 1;
    const int64_t field = (int64_t)C * 3 * vol.V;
    const float* d_last = c->steps + (int64_t)(cfg.no_steps - 1) * field;
    if (io->transformation || io->displacement) launch_svf_outputs(d_last, io->transformation, io->displacement, C, vol, lin, st);

    // regulariser energy -> loss terms, coefficients, hyper-parameter step.  For the L2 family the coefficient (w / 2) does not
    // depend on the energy, so the update kernel produces the energy as a by-product of its stencil and the scalar stage runs
    // after it, inside the finalize launch (same values in, same order of the hyper-parameter step: the update still sees the
    // w of this transition)
    const int upd_blocks = sgld_update_blocks_per_chain(volv, C);
    // the bending prior (bending_kernels.hip): its energy always comes first, whatever the knob says
    const bool bending = cfg.diff_op == IRS_DIFF_HESSIAN;
    const bool energy_in_update = !bending && (cfg.reg_loss == IRS_REG_L2 || cfg.reg_loss == IRS_REG_LOGNORMAL_L2) &&
                                  (int64_t)upd_blocks * C <= (int64_t)kMaxPartialBlocks * IRS_MAX_CHAINS &&
                                  c->kn.energy_in_update != 0;
    if (!energy_in_update) {
        if (bending) launch_bending_energy(vs, c->energy_partials, energy_blocks(volv), C, volv, st);
        else launch_reg_energy(vs, c->energy_partials, C, volv, st);
        launch_reg_scalar(c->state, c->energy_partials, energy_blocks(volv), c->dcfg, st, vd);
    }

    // per chain, serially (trainer.py:316-327): VD factor -> GMM step -> data term with the UPDATED mixture.  The serial part is the
    // mixture: the statistics of chain c + 1 need the parameters chain c's step left, and that step must not touch them while the
    // data term of chain c still reads them -- but the data term of chain c (a 36 us launch of 1024 workgroups at 128^3, alone on
    // the chip) and the statistics of chain c + 1 (24 us) only READ the same parameters: with `chain_overlap` the former runs on a
    // side stream, the next chain's scalar stage waits for it.  Same kernels, same inputs, same order of every sum: chains
    // bit-identical (tests/test_gpu_transition.py).  Measured SLOWER than the serial form (the two half-filled launches get in each
    // other's way and every chain pays two event hand-overs; profiles/r05_chain_overlap_ab.txt): off by default.
    //
    // `data_batch` (default): what the data term of chain c needs from the mixture are 2K derived constants -- chain c's scalar stage
    // leaves a snapshot of them (DevState::snapA), the serial loop is then statistics -> step only, and the data terms of ALL chains
    // run as one launch behind it (grid.z = segments x C: one launch that fills the chip instead of C half-filled ones, C - 1 launch
    // gaps less).  Same kernel arithmetic on the same values, same partial-sum slots: chains bit-identical to the serial form.
    const int sb = stats_blocks(vol);
    const bool overlap = C > 1 && c->side && c->kn.chain_overlap != 0;
    const bool batch = C > 1 && !overlap && cfg.data_loss == IRS_DATA_GMM_LCC && c->kn.data_batch != 0;
    for (int ch = 0; ch < C; ++ch) {
        const uint8_t* mask = io->mask + (io->mask_chains == 1 ? 0 : (int64_t)ch * vol.V);
        const float* zc = z + (int64_t)ch * vol.V;
        launch_stats(cfg.virtual_decimation, zc, mask, c->state, c->stat_partials, vol, st, c->dcfg.K);
        if (overlap && ch > 0) HIP_TRY(hipStreamWaitEvent(st, c->ev_side[2 * (ch - 1) + 1], 0));  // data term of chain ch - 1 has read the mixture
        launch_chain_scalar(c->state, c->stat_partials, sb, ch, (ch == 0 ? 7 : 3) | (batch ? 8 : 0), c->dcfg, st, vd);  // chain 0: + the verdict
        if (batch || data_on == 3 || lncc) continue;
        const float* f = cfg.data_loss == IRS_DATA_GMM_LCC ? c->fhat + (c->fhat_chains == 1 ? 0 : (int64_t)ch * vol.V) : nullptr;
        hipStream_t ds = st;
        if (overlap && ch + 1 < C) {  // (the last chain's data term has nothing to overlap with: it stays on the caller's stream)
            HIP_TRY(hipEventRecord(c->ev_side[2 * ch], st));
            HIP_TRY(hipStreamWaitEvent(c->side, c->ev_side[2 * ch], 0));
            ds = c->side;
        }
        launch_data_bwd(cfg.data_loss, f, 0, zc, c->sigM + (int64_t)ch * vol.V, mask, 0, nullptr, c->state, ch,
                        c->gM + (int64_t)ch * vol.V, c->nll_partials + (int64_t)ch * c->nll_blocks, cfg.lcc_s, 1, vol, ds, c->nll_seg_C);
        if (ds != st) HIP_TRY(hipEventRecord(c->ev_side[2 * ch + 1], c->side));
    }
    if (data_on == 3)  // (one chain, or all chains against their snapshots: scalar stage op bit 3 above)
        launch_lcc_data_bwd_plan(c->fhat, c->fhat_chains == 1 ? 0 : vol.V, z, c->sigM, io->mask, io->mask_chains == 1 ? 0 : vol.V, c->state, c->gM,
                                 cfg.lcc_s, C, vol, c->dplan, st);
    else if (mi)  // every chain in one launch: the tables of the forward pass -> g_warped (and mask * (ln B - pmi) for the caller)
        launch_mi_bwd(io->fixed_im, io->fixed_chains == 1 ? 0 : vol.V, warped, io->mask, io->mask_chains == 1 ? 0 : vol.V, c->mi_table, vol.V, C,
                      c->mi_bins, c->mi_weight, nullptr, true, c->gM, io->residuals, st);
    else if (ngf)  // every chain in one launch: weight * grad^T of the coefficient maps of the forward pass -> g_warped
        launch_ngf_bwd(c->ngf_coef, c->ngf_weight, c->gM, C, lncc_geometry(vol.D, vol.H, vol.W, 1), st);
    else if (lncc)  // every chain in one launch: the coefficient maps of the forward pass -> g_warped
        launch_lncc_bwd(io->fixed_im, io->fixed_chains == 1 ? 0 : vol.V, warped, c->lncc_coef, cfg.lcc_s, c->lncc_weight, c->gM, C,
                        lncc_geometry(vol.D, vol.H, vol.W, cfg.lcc_s), st);
    else if (batch)
        launch_data_bwd(cfg.data_loss, c->fhat, c->fhat_chains == 1 ? 0 : vol.V, z, c->sigM, io->mask, io->mask_chains == 1 ? 0 : vol.V, nullptr,
                        c->state, 0, c->gM, c->nll_partials, cfg.lcc_s, C, vol, st, c->nll_seg_C);
    // back through the warp and the squaring steps
    if (!fuse_warp_bwd)
        launch_warp_bwd(io->moving_im, io->moving_chains == 1 ? 0 : vol.V, d_last, io->unif,
                        cfg.uniform_alpha > 0.0f ? cfg.uniform_alpha : 0.0f, c->gM, c->gA, C, vol, lin, cfg.seed, 0, it, st);
    // the support of the gradient that enters the adjoint -> the piece lists of its steps (decided on the device: adjoint_plan.hip)
    // Only where pieces can get shorter than the full-column launch's segments: at 128^3 with one chain those are already the
    // shortest pieces (8 planes, one resident set), the lists could only match them, and the plan's four launches cost 3 % of that
    // transition (profiles/sparse_adjoint_ab.txt).  A launch-shape rule on sizes, like the segment lengths themselves.
    const bool sparse = c->sparse_adjoint && c->plan.entries != nullptr &&
                        (global_knobs().march_seg > 0 || exp_bwd_dense_seg_len(vol, C) > kPlanMinLen);
    c->plan_on = sparse;
    // (with the mask's extent table formed above the lists are cut from it, at the reach of g_warped's support around the mask more:
    // the same lists from transition to transition, and no pass over g_warped)
    const bool from_mask = data_on > 0 && !(c->sparse_plan & 2);
    if (sparse)
        launch_adjoint_plan(c->gM, from_mask ? &c->dplan : nullptr, io->mask_chains, lcc ? cfg.lcc_s : 0, c->dmax, c->plan, cfg.no_steps, C, vol,
                            exp_bwd_plan_resident(), global_knobs().march_seg, c->sparse_plan, st);
    LAUNCH_CHECK();
    if (timed) HIP_TRY(hipEventRecord(c->ev[3], st));
    const float* dense = c->ffd ? c->dense : vs;
    float* g0 = nullptr;
    {
        // the adjoint ping-pongs between two buffers; the incoming gradient sits in gA, so start writing into gB
        const float* G = c->gA;
        float* bufs[2] = {c->gB, c->gA};
        int cur = 0;
        for (int k = cfg.no_steps - 1; k >= 0; --k) {
            float* out = bufs[cur];
            const float* dk = k == 0 ? dense : c->steps + (int64_t)(k - 1) * field;
            if (timed) HIP_TRY(hipEventRecord(c->ev_bwd[2 * k], st));
            const unsigned* dm = c->dmax + (int64_t)k * C * 4;
            // fused backward warp: gA holds d(warped)/d(d_last); the first step scales it by g_warped while staging
            const float* gscale = fuse_warp_bwd && k == cfg.no_steps - 1 ? c->gM : nullptr;
            // with the fused backward warp the first step's incoming gradient is the interleaved d(warped)/d(d_n)
            const int lay = bwd_lay(c, k) | (gscale ? 2 : 0);
            const bool sa = k < 32 && skip_any[k], s2 = k < 32 && skip_r2[k];
            // timed mode: the end event of step k closes right after the radius-1 kernel, so that exp_bwd_kernel_ms is the time
            // of the dominant kernel alone (as rocprofv3 reports it), not of the idle variants after it
            // lds_from 2: the any-radius kernel, when launched, takes every step beyond the radius-1 gather (no radius-2 gather then)
            const int gr = global_knobs().lds_from <= 2 ? 1 : 2;
            launch_exp_step_bwd_march(G, dk, out, k == 0, cfg.no_steps, C, vol, lin, dm, (s2 || (gr == 1 && !sa)) ? 1 : 2, sa, gscale, lay,
                                      timed ? c->ev_bwd[2 * k + 1] : nullptr, st, sparse ? &c->plan : nullptr, k);
            if (!sa) launch_exp_step_bwd_lds(G, dk, out, k == 0, cfg.no_steps, C, vol, lin, dm, 2, gr, gscale, lay, c->cmm, st);
            G = out;
            cur ^= 1;
        }
        g0 = const_cast<float*>(G);
    }
    if (timed) HIP_TRY(hipEventRecord(c->ev[4], st));
    float s[3];
    prescale_factors(vol, cfg.no_steps, s);
    // SGHMC (irs_sghmc_set): the same launches, the step of sghmc_device.h in place of v <- v - lr grad_v
    const SghmcArgs hm_args = sghmc_args(c->sghmc_m, io->eps, cfg.lr, c->sghmc_friction, c->sghmc_temperature, cfg.seed);
    const SghmcArgs* hm = c->sghmc ? &hm_args : nullptr;
    if (c->ffd) {
        float* scaled = g0 == c->gA ? c->gB : c->gA;
        launch_scale_channels(g0, scaled, s[0], s[1], s[2], C, vol, st);
        const int G[3] = {volv.D, volv.H, volv.W};
        ffd_adjoint(scaled, c->tmpB, c->tmpA, C, vol, G, c->spl, st);
        if (bending) launch_sgld_update_bending(io->v, io->sigma, c->tmpB, vs, c->state, cfg.lr, 1.0f, 1.0f, 1.0f, io->grad_v, C, volv, st, hm);
        else launch_sgld_update(io->v, io->sigma, c->tmpB, vs, c->state, cfg.lr, 1.0f, 1.0f, 1.0f, io->grad_v, C, volv, st,
                                energy_in_update ? c->energy_partials : nullptr, energy_in_update, hm);
    } else if (bending) {
        launch_sgld_update_bending(io->v, io->sigma, g0, vs, c->state, cfg.lr, s[0], s[1], s[2], io->grad_v, C, volv, st, hm);
    } else {
        launch_sgld_update(io->v, io->sigma, g0, vs, c->state, cfg.lr, s[0], s[1], s[2], io->grad_v, C, volv, st,
                           energy_in_update ? c->energy_partials : nullptr, energy_in_update, hm);
    }
    // bookkeeping (+ the regulariser scalar stage of the L2 family, whose energy the update has just produced: one launch)
    launch_finalize(c->state, data_on == 3 ? c->dplan.nll : c->nll_partials, c->nll_blocks, c->dcfg, true, c->dmax, c->hint,
                    4 * C * (cfg.no_steps + 1), vd, kHintWords - 7, true, st, energy_in_update ? c->energy_partials : nullptr, upd_blocks,
                    data_on == 3 ? c->dplan.entries : nullptr, data_on == 3 ? c->dplan.count : nullptr);
    c->dmax_clean = true;
    LAUNCH_CHECK();
    if (timed) HIP_TRY(hipEventRecord(c->ev[5], st));
    // (under stream capture nothing has been enqueued on the device -- the launch sequence became graph nodes, and an event
    // recorded inside a capture cannot be waited for by the host: the run-ahead bookkeeping counts executed transitions only)
    if (is_capturing(st)) return 0;
    HIP_TRY(hipEventRecord(c->ra_ev[c->n_enqueued % 4], st));
    ++c->n_enqueued;
    return 0;
}

// failed (no-op) transitions the device has reported since the host last looked -> transitions to re-run
static void poll_failures(irs_ctx* c) {
    if (!c->hint) return;
    const unsigned f = ((volatile unsigned*)c->hint)[kHintWords - 7];
    if (f == c->fails_seen || (int)(f - c->fails_seen) < 0) return;  // (a count that went backwards is not 4e9 failures)
    c->makeup += (uint64_t)(f - c->fails_seen);
    c->fails_total += (uint64_t)(f - c->fails_seen);
    c->fails_seen = f;
    // the bounds that misled the prediction are still the ones the host sees: no assumptions for the next few transitions
    c->force_all_until = c->n_enqueued + c->makeup + 3;
}

static void drop_pending(irs_ctx* c) {
    poll_failures(c);
    c->makeup = 0;
}

static int transition_impl(irs_ctx* c, const irs_io* io, hipStream_t st, int timed) {
    if (check_io(c, io, "irs_transition")) return 1;
    if (!io->v) return fail("irs_transition: v is required");
    // Under stream capture the launch sequence becomes a graph that is replayed without this host code: no prediction may be
    // baked into it (a replay whose verdict failed would stay a no-op on every replay) and no pending re-run belongs in it.
    if (is_capturing(st)) {
        // (timing events are read back by the host right after the call, which a captured stream never executed: refused.
        // The io of this call is still "the last one": irs_flush re-runs with it.)
        if (timed) return fail("irs_transition_timed: the stream is being captured -- per-stage timings need a stream that executes");
        c->last_io = *io;
        c->have_last_io = true;
        return enqueue_transition(c, io, st, 0, true);
    }
    // Bounded run-ahead: the host may be at most IRS_RUN_AHEAD (default 2) transitions ahead of the device.  The variant
    // prediction reads bounds the device published at the end of an earlier transition; a host that has queued twenty
    // transitions would predict from a state twenty transitions old, and while the displacement is still growing (burn-in)
    // that mispredicts into the slow always-correct fallbacks.  Two queued transitions keep the device busy all the same.
    const int depth = c->kn.run_ahead;
    if (depth > 0 && depth <= 3 && c->n_enqueued >= (uint64_t)depth) HIP_TRY(hipEventSynchronize(c->ra_ev[(c->n_enqueued - depth) % 4]));
    // A transition whose assumptions about max|d_k| failed was a no-op on the device (nothing changed, the Philox counter did
    // not advance): it is re-run here, without assumptions, before the transition of this call -- the chain continues as if
    // every variant had been launched all along (same noise, same order; with injected eps / unif the re-run uses THIS call's).
    poll_failures(c);
    if (c->makeup && !c->kn.recover)
        return fail("irs_transition: an earlier transition skipped a kernel variant its displacement then needed and was dropped "
                    "(recover = 0); predict_variants = 0 launches every variant");
    while (c->makeup > 0) {
        --c->makeup;
        if (enqueue_transition(c, io, st, 0, true)) return 1;
    }
    c->last_io = *io;
    c->have_last_io = true;
    return enqueue_transition(c, io, st, timed, c->n_enqueued < c->force_all_until);
}

// wait for everything enqueued, then re-run what failed (with the io of the last call); afterwards state, scalars and v are final
static int flush_impl(irs_ctx* c, hipStream_t st) {
    for (int guard = 0; guard < 8; ++guard) {
        HIP_TRY(hipStreamSynchronize(st));
        if (c->n_enqueued) HIP_TRY(hipEventSynchronize(c->ra_ev[(c->n_enqueued - 1) % 4]));
        poll_failures(c);
        if (!c->makeup) return 0;
        if (!c->kn.recover || !c->have_last_io) return fail("irs_flush: %llu transition(s) were dropped after a failed variant prediction", (unsigned long long)c->makeup);
        while (c->makeup > 0) {
            --c->makeup;
            if (enqueue_transition(c, &c->last_io, st, 0, true)) return 1;
        }
    }
    return fail("irs_flush: transitions keep failing");
}

int irs_flush(irs_ctx* c, void* stream) {
    if (!c) return fail("irs_flush: null argument");
    if (c->sl.on) return irs::slab_flush(c, (hipStream_t)stream);
    return flush_impl(c, (hipStream_t)stream);
}

int irs_recovered_transitions(const irs_ctx* c, uint64_t* out) {
    if (!c || !out) return fail("irs_recovered_transitions: null argument");
    *out = c->fails_total;
    return 0;
}

int irs_sparse_adjoint_set(irs_ctx* c, int on) {
    if (!c) return fail("irs_sparse_adjoint_set: null argument");
    c->sparse_adjoint = on != 0;
    return 0;
}

int irs_sparse_adjoint_get(irs_ctx* c, int32_t* out, void* stream) {
    if (!c || !out) return fail("irs_sparse_adjoint_get: null argument");
    const size_t n = (size_t)c->cfg.no_steps * c->C * kPlanStats;
    memset(out, 0, n * sizeof(int32_t));
    if (!c->plan.stats || !c->plan_on || c->n_enqueued == 0) return 0;  // full columns: nothing engaged
    if (irs_flush(c, stream)) return 1;
    HIP_TRY(hipMemcpyAsync(out, c->plan.stats, n * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int irs_sparse_plan_set(irs_ctx* c, int reuse) {
    if (!c) return fail("irs_sparse_plan_set: null argument");
    if (reuse < 0 || reuse > 3) return fail("irs_sparse_plan_set: bit 0 reuse, bit 1 the adjoint's lists from the gradient");
    c->sparse_plan = reuse;
    return 0;
}

int irs_lncc_set(irs_ctx* c, float weight, float eps) {
    if (!c) return fail("irs_lncc_set: null argument");
    if (c->cfg.data_loss != IRS_DATA_LNCC) return fail("irs_lncc_set: the context's data loss is not IRS_DATA_LNCC");
    if (!positive_finite(weight) || !positive_finite(eps))
        return fail("irs_lncc_set: weight = %g, eps = %g, finite values > 0 needed", (double)weight, (double)eps);
    if (c->n_enqueued > 0 || c->have_last_io) return fail("irs_lncc_set: weight and eps may be set only before the first transition");
    c->lncc_weight = weight;
    c->lncc_eps = eps;
    return 0;
}

int irs_sghmc_set(irs_ctx* c, float friction, float temperature, float* momentum) {
    if (!c || !momentum) return fail("irs_sghmc_set: null argument");
    if (c->sl.on) return fail("irs_sghmc_set: a z-slab context keeps the reference's update");
    if (!sghmc_numbers_ok("irs_sghmc_set", friction, temperature)) return 1;
    if (c->n_enqueued > 0 || c->have_last_io) return fail("irs_sghmc_set: the sampler may be set only before the first transition");
    c->sghmc = true;
    c->sghmc_friction = friction;
    c->sghmc_temperature = temperature;
    c->sghmc_m = momentum;
    return 0;
}

int irs_mi_set(irs_ctx* c, float weight, float f_lo, float f_hi, float m_lo, float m_hi) {
    if (!c) return fail("irs_mi_set: null argument");
    if (c->cfg.data_loss != IRS_DATA_MI) return fail("irs_mi_set: the context's data loss is not IRS_DATA_MI");
    if (!positive_finite(weight)) return fail("irs_mi_set: weight = %g, a finite value > 0 needed", (double)weight);
    if (c->n_enqueued > 0 || c->have_last_io) return fail("irs_mi_set: weight and ranges may be set only before the first transition");
    MiBins bn;
    if (!mi_bins_ok("irs_mi_set", c->cfg.lcc_s, f_lo, f_hi, m_lo, m_hi, bn)) return 1;
    c->mi_bins = bn;
    c->mi_weight = weight;
    c->mi_set = true;
    return 0;
}

int irs_ngf_set(irs_ctx* c, float weight, float eps_f, float eps_m) {
    if (!c) return fail("irs_ngf_set: null argument");
    if (c->cfg.data_loss != IRS_DATA_NGF) return fail("irs_ngf_set: the context's data loss is not IRS_DATA_NGF");
    if (!positive_finite(weight) || !positive_finite(eps_f) || !positive_finite(eps_m))
        return fail("irs_ngf_set: weight = %g, eps_f = %g, eps_m = %g, finite values > 0 needed", (double)weight, (double)eps_f, (double)eps_m);
    if (c->n_enqueued > 0 || c->have_last_io) return fail("irs_ngf_set: weight and edge parameters may be set only before the first transition");
    c->ngf_weight = weight;
    c->ngf_eps_f = eps_f;
    c->ngf_eps_m = eps_m;
    c->ngf_set = true;
    return 0;
}

int irs_sparse_plan_get(irs_ctx* c, int32_t* out, void* stream) {
    if (!c || !out) return fail("irs_sparse_plan_get: null argument");
    memset(out, 0, 6 * sizeof(int32_t));
    if (!c->plan.counters || c->n_enqueued == 0) return 0;
    if (irs_flush(c, stream)) return 1;
    const int* src[3] = {c->dplan.counters, c->fplan.counters, c->plan.counters};
    for (int i = 0; i < 3; ++i)
        if (src[i]) HIP_TRY(hipMemcpyAsync(out + 2 * i, src[i], 2 * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int irs_sparse_forward_set(irs_ctx* c, int on) {
    if (!c) return fail("irs_sparse_forward_set: null argument");
    if (on < 0) return fail("irs_sparse_forward_set: 0 (off), 1 (on) or a piece length");
    c->sparse_forward = on;
    return 0;
}

int irs_sparse_forward_get(irs_ctx* c, int32_t* out, void* stream) {
    if (!c || !out) return fail("irs_sparse_forward_get: null argument");
    const int n = c->cfg.no_steps, C = c->C;
    memset(out, 0, (size_t)n * C * kForwardStats * sizeof(int32_t));
    if (!c->fplan.stats || !c->fwd_on || c->n_enqueued == 0) return 0;  // dense forward steps: nothing engaged
    int width[32];  // (a re-run inside irs_flush is dense and clears fwd_on: the figures are those of the last transition CALLED)
    memcpy(width, c->fwd_width, sizeof(width));
    if (irs_flush(c, stream)) return 1;
    int32_t stats[32 * IRS_MAX_CHAINS * kPlanStats];
    HIP_TRY(hipMemcpyAsync(stats, c->fplan.stats, (size_t)n * C * kPlanStats * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < n * C; ++i) {
        memcpy(out + (size_t)i * kForwardStats, stats + (size_t)i * kPlanStats, sizeof(int32_t) * kPlanStats);
        out[(size_t)i * kForwardStats + kPlanStats] = width[i / C];
    }
    return 0;
}

int irs_sparse_data_set(irs_ctx* c, int on) {
    if (!c) return fail("irs_sparse_data_set: null argument");
    if (on < 0) return fail("irs_sparse_data_set: 0 (off), 1 (on) or a piece length");
    c->sparse_data = on;
    return 0;
}

int irs_sparse_data_get(irs_ctx* c, int32_t* out, void* stream) {
    if (!c || !out) return fail("irs_sparse_data_get: null argument");
    const int C = c->C;
    memset(out, 0, (size_t)kDataKernels * C * kPlanStats * sizeof(int32_t));
    if (!c->dplan.entries || c->data_on == 0 || c->n_enqueued == 0) return 0;  // the dense stage: nothing engaged
    if (irs_flush(c, stream)) return 1;
    // row 0 (warp: no list): the tile-planes of 64 x 8 inside the hull; rows 1 / 3 (map, data term): the lists' own figures; row 2
    // (statistics): zero -- trimming its segments to the hull measured no faster, it keeps its dense launch
    const size_t tiles = (size_t)c->dplan.wtx * c->dplan.wty;
    int* hull = (int*)malloc(sizeof(int) * 2 * tiles * C);
    int32_t lists[2 * IRS_MAX_CHAINS * kPlanStats];
    if (!hull) return fail("irs_sparse_data_get: out of host memory");
    hipError_t e = hipMemcpyAsync(hull, c->dplan.hull, sizeof(int) * 2 * tiles * C, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lists, c->dplan.stats, sizeof(int32_t) * 2 * C * kPlanStats, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) {
        free(hull);
        return fail("irs_sparse_data_get: read-back failed: %s", hipGetErrorString(e));
    }
    for (int ch = 0; ch < C; ++ch) {
        int32_t planes = 0;
        for (size_t t = 0; t < tiles; ++t) planes += hull[(ch * tiles + t) * 2 + 1] - hull[(ch * tiles + t) * 2];
        out[(size_t)ch * kPlanStats] = 1;
        out[(size_t)ch * kPlanStats + 3] = planes;
        if (c->data_on >= 2) memcpy(out + ((size_t)1 * C + ch) * kPlanStats, lists + ((size_t)C + ch) * kPlanStats, sizeof(int32_t) * kPlanStats);
        if (c->data_on >= 3) memcpy(out + ((size_t)3 * C + ch) * kPlanStats, lists + (size_t)ch * kPlanStats, sizeof(int32_t) * kPlanStats);
    }
    free(hull);
    return 0;
}

int irs_transition(irs_ctx* c, const irs_io* io, void* stream) { return transition_impl(c, io, (hipStream_t)stream, 0); }

int irs_transition_timed(irs_ctx* c, const irs_io* io, void* stream, irs_timings* out) {
    if (!out) return fail("irs_transition_timed: null output");
    if (c && c->cfg.no_steps > 32) return fail("irs_transition_timed: at most 32 steps");
    if (transition_impl(c, io, (hipStream_t)stream, 1)) return 1;
    HIP_TRY(hipEventSynchronize(c->ev[5]));
    memset(out, 0, sizeof(*out));
    HIP_TRY(hipEventElapsedTime(&out->total_ms, c->ev[0], c->ev[5]));
    HIP_TRY(hipEventElapsedTime(&out->smooth_ms, c->ev[0], c->ev[1]));
    HIP_TRY(hipEventElapsedTime(&out->exp_fwd_ms, c->ev[1], c->ev[2]));
    HIP_TRY(hipEventElapsedTime(&out->data_ms, c->ev[2], c->ev[3]));
    HIP_TRY(hipEventElapsedTime(&out->exp_bwd_total_ms, c->ev[3], c->ev[4]));
    HIP_TRY(hipEventElapsedTime(&out->update_ms, c->ev[4], c->ev[5]));
    for (int k = 0; k < c->cfg.no_steps; ++k) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_bwd[2 * k], c->ev_bwd[2 * k + 1]));
        out->exp_bwd_kernel_ms += ms;
        if (k >= 1) out->exp_bwd_primary_avg_ms += ms / (float)(c->cfg.no_steps > 1 ? c->cfg.no_steps - 1 : 1);
    }
    return 0;
}

}  // extern "C"
