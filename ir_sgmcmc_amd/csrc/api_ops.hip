// C ABI (include/irsgmcmc.h), the stateless part: the error plumbing and every operator and diagnostic that needs no context --
// argument validation (api_checks.h), workspace layout, launches.  No exceptions / aborts cross this boundary; errors come back
// as codes + irs_last_error().  The switches are in knobs.hip, the context and the SG-MCMC transition in api_ctx.hip.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "api_checks.h"

using namespace irs;

namespace irs {

static thread_local char g_err[512] = "";

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

// `dense` / `g_dense` hold the planes [store_lo, store_lo + store_n) of the volume (whole volume: 0, D); up-sampling produces the
// planes [w_lo, w_lo + w_n), the adjoint sums over them (a rank's own planes: partial control-grid gradients, all-reduced)
int ffd_up(const float* v_cp, float* dense, float* tmp, int C, Vol vol, const int G[3], const SplineTaps spl[3], hipStream_t st,
           int w_lo, int w_n, int store_lo, int store_n) {
    // axis order of utils/transformation.py:146-149: tensor axis 2 (D, cps[0]), 3 (H, cps[1]), 4 (W, cps[2])
    if (w_n < 0) { w_lo = 0; w_n = vol.D; }
    if (store_n < 0) { store_lo = 0; store_n = vol.D; }
    const int64_t CC = (int64_t)C * 3;
    float* t1 = tmp;
    float* t2 = tmp + CC * store_n * G[1] * G[2];
    launch_ffd_axis(v_cp, t1, spl[0], false, CC, G[0], vol.D, (int64_t)G[1] * G[2], st, w_lo, w_n, store_lo, store_n);
    launch_ffd_axis(t1, t2, spl[1], false, CC * store_n, G[1], vol.H, G[2], st);
    launch_ffd_axis(t2, dense, spl[2], false, CC * store_n * vol.H, G[2], vol.W, 1, st);
    return 0;
}

int ffd_adjoint(const float* g_dense, float* g_cp, float* tmp, int C, Vol vol, const int G[3], const SplineTaps spl[3],
                hipStream_t st, int w_lo, int w_n, int store_lo, int store_n) {
    if (w_n < 0) { w_lo = 0; w_n = vol.D; }
    if (store_n < 0) { store_lo = 0; store_n = vol.D; }
    const int64_t CC = (int64_t)C * 3;
    float* t1 = tmp;
    float* t2 = tmp + CC * store_n * vol.H * G[2];
    launch_ffd_axis(g_dense, t1, spl[2], true, CC * store_n * vol.H, vol.W, G[2], 1, st);
    launch_ffd_axis(t1, t2, spl[1], true, CC * store_n, vol.H, G[1], G[2], st);
    launch_ffd_axis(t2, g_cp, spl[0], true, CC, vol.D, G[0], (int64_t)G[1] * G[2], st, w_lo, w_n, store_lo, store_n);
    return 0;
}

}  // namespace irs

extern "C" {

const char* irs_last_error(void) { return irs::g_err; }
const char* irs_version(void) { return "ir-sgmcmc-amd 0.1 (gfx950)"; }
size_t irs_reduce_scratch_doubles(void) { return (size_t)kMaxPartialBlocks * IRS_MAX_CHAINS; }

// ================================================================================================
// stateless operators
// ================================================================================================

int irs_perturb_smooth(const float* v, const float* sigma, const float* eps, float tau, const float* kernel, int s,
                       int C, int D, int H, int W, float* tmp, float* out, uint64_t seed, uint64_t iteration,
                       void* stream) {
    if (!v || !out || !dims_ok(C, D, H, W)) return fail("irs_perturb_smooth: bad arguments");
    if (s < 0 || s > IRS_MAX_HALF_WIDTH || (s > 0 && (!kernel || !tmp))) return fail("irs_perturb_smooth: bad kernel/s");
    hipStream_t st = (hipStream_t)stream;
    const Vol vol = make_vol(D, H, W);
    const size_t bytes = (size_t)C * 3 * vol.V * sizeof(float);
    if (s == 0) {
        if (tau >= 0.0f) launch_perturb(v, sigma, eps, sqrtf(2.0f * tau), out, C, vol, seed, iteration, nullptr, st);
        else HIP_TRY(hipMemcpyAsync(out, v, bytes, hipMemcpyDeviceToDevice, st));
        LAUNCH_CHECK();
        return 0;
    }
    Taps taps;
    taps.s = s;
    for (int i = 0; i <= 2 * s; ++i) taps.k[i] = kernel[i];
    const float* src = v;
    if (tau >= 0.0f && global_knobs().fuse_noise) {  // the noise is generated while the smoothing kernel stages its planes
        launch_perturb_sobolev_march(v, sigma, eps, (float)sqrt(2.0 * (double)tau), out, taps, C, vol, nullptr, 12, seed, iteration, nullptr, st);
        LAUNCH_CHECK();
        return 0;
    }
    if (tau >= 0.0f) {
        launch_perturb(v, sigma, eps, (float)sqrt(2.0 * (double)tau), out, C, vol, seed, iteration, nullptr, st);
        src = out;
    }
    if (src == out) {  // the marching kernel cannot run in place
        HIP_TRY(hipMemcpyAsync(tmp, out, bytes, hipMemcpyDeviceToDevice, st));
        src = tmp;
    }
    launch_sobolev_march(src, out, taps, C * 3, vol, nullptr, 12, st);
    LAUNCH_CHECK();
    return 0;
}

int irs_sghmc_update(float* v, float* momentum, const float* grad, const float* sigma, const float* eps, int C, int D, int H, int W,
                     float lr, float friction, float temperature, uint64_t seed, uint64_t iteration, void* stream) {
    if (!v || !momentum || !grad) return fail("irs_sghmc_update: null argument");
    if (D < 1 || H < 1 || W < 1) return fail("irs_sghmc_update: dims (%d, %d, %d), every one >= 1 needed", D, H, W);
    if (!chains_ok("irs_sghmc_update", C)) return 1;
    if (!sghmc_numbers_ok("irs_sghmc_update", friction, temperature)) return 1;
    if (!isfinite(lr) || lr < 0.0f) return fail("irs_sghmc_update: lr = %g, a finite value >= 0 needed", (double)lr);
    if ((int64_t)D * H * W >= ((int64_t)1 << 30)) return fail("irs_sghmc_update: the volume must have fewer than 2^30 voxels");
    // one block row per (chain, plane pair) and per four rows of a plane
    if ((int64_t)((D + 1) / 2) * C > 65535 || (H + 3) / 4 > 65535)
        return fail("irs_sghmc_update: dims (%d, %d, %d) x %d chains exceed the launch grid", D, H, W, C);
    launch_sghmc_update(v, grad, sigma, lr, sghmc_args(momentum, eps, lr, friction, temperature, seed), iteration, C, make_vol(D, H, W),
                        (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_svf_exp_fwd(const float* v, float* steps, float* transformation, float* displacement, int no_steps, int C,
                    int D, int H, int W, void* stream) {
    if (!v || !steps || !dims_ok(C, D, H, W) || no_steps < 1 || no_steps > 30) return fail("irs_svf_exp_fwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const Vol vol = make_vol(D, H, W);
    Lin lin;
    if (cached_lin(D, H, W, st, &lin)) return fail("irs_svf_exp_fwd: identity grid allocation failed");
    const int64_t field = (int64_t)C * 3 * vol.V;
    for (int k = 0; k < no_steps; ++k) {
        const float* in = k == 0 ? v : steps + (int64_t)(k - 1) * field;
        launch_exp_step_fwd_march(in, steps + (int64_t)k * field, k == 0, no_steps, C, vol, lin, nullptr, nullptr, false, 0, st);
    }
    if (transformation || displacement)
        launch_svf_outputs(steps + (int64_t)(no_steps - 1) * field, transformation, displacement, C, vol, lin, st);
    LAUNCH_CHECK();
    return 0;
}

static int exp_backward(const float* v, const float* steps, const float* g_last, float* gA, float* gB, int no_steps, int C,
                        Vol vol, Lin lin, hipStream_t st, float** result) {
    const int64_t field = (int64_t)C * 3 * vol.V;
    const float* G = g_last;
    float* bufs[2] = {gA, gB};
    int cur = 0;
    // Scratch of the stateless operator, one set PER DEVICE (a pointer of device 0 is no use to a launch on device 1), guarded
    // by a mutex and regrown only after the WHOLE device has drained (another stream may still be reading the old block).
    // [32 steps][8 chains][4] bounds + the coarse displacement extrema of the any-radius adjoint (kernels.h).
    struct Scratch {
        unsigned* dmax = nullptr;
        float* cmm = nullptr;
        size_t cmm_bytes = 0;
    };
    static Scratch per_device[64];
    static std::mutex mu;
    int dev_id = 0;
    HIP_TRY(hipGetDevice(&dev_id));
    if (dev_id < 0 || dev_id >= 64) return fail("irs_svf_exp_bwd: device ordinal %d out of range", dev_id);
    unsigned* dmax;
    float* cmm;
    {
        std::lock_guard<std::mutex> lock(mu);
        Scratch& sc = per_device[dev_id];
        if (!sc.dmax) HIP_TRY(hipMalloc((void**)&sc.dmax, sizeof(unsigned) * 4 * IRS_MAX_CHAINS * 32));
        if (coarse_minmax_bytes(vol, C) > sc.cmm_bytes) {
            HIP_TRY(hipDeviceSynchronize());
            if (sc.cmm) HIP_TRY(hipFree(sc.cmm));
            sc.cmm = nullptr;
            sc.cmm_bytes = 0;
            HIP_TRY(hipMalloc((void**)&sc.cmm, coarse_minmax_bytes(vol, C)));
            sc.cmm_bytes = coarse_minmax_bytes(vol, C);
        }
        dmax = sc.dmax;
        cmm = sc.cmm;
    }
    if (C > IRS_MAX_CHAINS || no_steps > 32) return fail("irs_svf_exp_bwd: at most %d chains / 32 steps", IRS_MAX_CHAINS);
    HIP_TRY(hipMemsetAsync(dmax, 0, sizeof(unsigned) * 4 * IRS_MAX_CHAINS * 32, st));
    for (int k = no_steps - 1; k >= 0; --k) {
        float* out = bufs[cur];
        const float* dk = k == 0 ? v : steps + (int64_t)(k - 1) * field;
        // every variant is launched (radius-1 / radius-2 gather, any-radius fixed-point scatter); the device picks by max|d_k|
        launch_field_absmax(dk, k == 0, no_steps, dmax + (int64_t)k * IRS_MAX_CHAINS * 4, C, vol, st);
        launch_exp_step_bwd_march(G, dk, out, k == 0, no_steps, C, vol, lin, dmax + (int64_t)k * IRS_MAX_CHAINS * 4, 2, false, nullptr, 0, nullptr, st);
        launch_exp_step_bwd_lds(G, dk, out, k == 0, no_steps, C, vol, lin, dmax + (int64_t)k * IRS_MAX_CHAINS * 4, 2, 2, nullptr, 0, cmm, st);
        G = out;
        cur ^= 1;
    }
    *result = const_cast<float*>(G);
    return 0;
}

int irs_svf_exp_bwd(const float* v, const float* steps, const float* g_last, float* scratch, float* g_v, int no_steps,
                    int C, int D, int H, int W, void* stream) {
    if (!v || !steps || !g_last || !scratch || !g_v || !dims_ok(C, D, H, W) || no_steps < 1 || no_steps > 30)
        return fail("irs_svf_exp_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const Vol vol = make_vol(D, H, W);
    Lin lin;
    if (cached_lin(D, H, W, st, &lin)) return fail("irs_svf_exp_bwd: identity grid allocation failed");
    const int64_t field = (int64_t)C * 3 * vol.V;
    float* res = nullptr;
    if (exp_backward(v, steps, g_last, scratch, scratch + field, no_steps, C, vol, lin, st, &res)) return 1;
    float s[3];
    prescale_factors(vol, no_steps, s);
    launch_scale_channels(res, g_v, s[0], s[1], s[2], C, vol, st);
    LAUNCH_CHECK();
    return 0;
}

static bool ffd_args_ok(int C, int D, int H, int W, int c0, int c1, int c2) {
    return dims_ok(C, D, H, W) && c0 >= 1 && c1 >= 1 && c2 >= 1 && c0 <= 8 && c1 <= 8 && c2 <= 8;
}

// the two intermediates of ffd_up / ffd_adjoint above: (C,3,D,G1,G2) and (C,3,D,H,G2), in either direction
size_t irs_ffd_scratch_floats(int C, int D, int H, int W, int c0, int c1, int c2) {
    if (!ffd_args_ok(C, D, H, W, c0, c1, c2)) return 0;
    const size_t G1 = (size_t)control_points(H, c1), G2 = (size_t)control_points(W, c2);
    return (size_t)C * 3 * (size_t)D * (G1 * G2 + (size_t)H * G2);
}

int irs_ffd_up(const float* v_cp, float* dense, float* tmp, int C, int D, int H, int W, int c0, int c1, int c2,
               void* stream) {
    if (!v_cp || !dense || !tmp || !ffd_args_ok(C, D, H, W, c0, c1, c2))
        return fail("irs_ffd_up: bad arguments");
    const Vol vol = make_vol(D, H, W);
    const int G[3] = {control_points(D, c0), control_points(H, c1), control_points(W, c2)};
    const SplineTaps spl[3] = {make_spline(c0), make_spline(c1), make_spline(c2)};
    ffd_up(v_cp, dense, tmp, C, vol, G, spl, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_ffd_adjoint(const float* g_dense, float* g_cp, float* tmp, int C, int D, int H, int W, int c0, int c1, int c2,
                    void* stream) {
    if (!g_dense || !g_cp || !tmp || !ffd_args_ok(C, D, H, W, c0, c1, c2))
        return fail("irs_ffd_adjoint: bad arguments");
    const Vol vol = make_vol(D, H, W);
    const int G[3] = {control_points(D, c0), control_points(H, c1), control_points(W, c2)};
    const SplineTaps spl[3] = {make_spline(c0), make_spline(c1), make_spline(c2)};
    ffd_adjoint(g_dense, g_cp, tmp, C, vol, G, spl, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_warp_fwd(const float* im, int Cim, const float* d_last, const float* unif, float alpha, float* warped, int C,
                 int D, int H, int W, uint64_t seed, uint64_t iteration, void* stream) {
    if (!im || !d_last || !warped || !dims_ok(C, D, H, W) || !broadcast_ok(Cim, C)) return fail("irs_warp_fwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const Vol vol = make_vol(D, H, W);
    Lin lin;
    if (cached_lin(D, H, W, st, &lin)) return fail("irs_warp_fwd: identity grid allocation failed");
    launch_warp_fwd(im, Cim == 1 ? 0 : vol.V, d_last, unif, alpha, warped, nullptr, 0, C, vol, lin, seed, iteration, nullptr, st);
    LAUNCH_CHECK();
    return 0;
}

int irs_warp_bwd(const float* im, int Cim, const float* d_last, const float* unif, float alpha, const float* g_warped,
                 float* g_d, int C, int D, int H, int W, uint64_t seed, uint64_t iteration, void* stream) {
    if (!im || !d_last || !g_warped || !g_d || !dims_ok(C, D, H, W) || !broadcast_ok(Cim, C))
        return fail("irs_warp_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const Vol vol = make_vol(D, H, W);
    Lin lin;
    if (cached_lin(D, H, W, st, &lin)) return fail("irs_warp_bwd: identity grid allocation failed");
    launch_warp_bwd(im, Cim == 1 ? 0 : vol.V, d_last, unif, alpha, g_warped, g_d, C, vol, lin, seed, iteration, nullptr, st);
    LAUNCH_CHECK();
    return 0;
}

int irs_warp_transformation(const float* im, int Cim, const float* transformation, float* warped, int C, int D, int H,
                            int W, void* stream) {
    if (!im || !transformation || !warped || !dims_ok(C, D, H, W) || !broadcast_ok(Cim, C))
        return fail("irs_warp_transformation: bad arguments");
    const Vol vol = make_vol(D, H, W);
    launch_warp_transformation(im, Cim == 1 ? 0 : vol.V, transformation, warped, C, vol, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_warp_nearest_u8(const uint8_t* seg, int Cim, const float* transformation, uint8_t* out, int C, int D, int H,
                        int W, void* stream) {
    if (!seg || !transformation || !out || !dims_ok(C, D, H, W) || !broadcast_ok(Cim, C))
        return fail("irs_warp_nearest_u8: bad arguments");
    const Vol vol = make_vol(D, H, W);
    launch_warp_nearest_u8(seg, Cim == 1 ? 0 : vol.V, transformation, out, C, vol, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_warp_nearest_i16(const int16_t* seg, int Cim, const float* transformation, int16_t* out, int C, int D, int H,
                         int W, void* stream) {
    if (!seg || !transformation || !out || !dims_ok(C, D, H, W) || !broadcast_ok(Cim, C))
        return fail("irs_warp_nearest_i16: bad arguments");
    const Vol vol = make_vol(D, H, W);
    launch_warp_nearest_i16(seg, Cim == 1 ? 0 : vol.V, transformation, out, C, vol, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_lcc_normalise(const float* im, float* out, float* sigma_out, int s, int C, int D, int H, int W, void* stream) {
    if (!im || !out || !dims_ok(C, D, H, W)) return fail("irs_lcc_normalise: bad arguments");
    if (!lcc_ok(s, D, H, W)) return fail("irs_lcc_normalise: LCC half width must be 1 or 2 and smaller than half the volume");
    launch_lcc_fwd_march(nullptr, 0, im, out, sigma_out, s, C, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_lcc_map_fwd(const float* fhat, int Cf, const float* warped, float* z, float* sigma_m, int s, int C, int D,
                    int H, int W, void* stream) {
    if (!fhat || !warped || !z || !sigma_m || !dims_ok(C, D, H, W) || !broadcast_ok(Cf, C))
        return fail("irs_lcc_map_fwd: bad arguments");
    if (!lcc_ok(s, D, H, W)) return fail("irs_lcc_map_fwd: LCC half width must be 1 or 2 and smaller than half the volume");
    const Vol vol = make_vol(D, H, W);
    launch_lcc_fwd_march(fhat, Cf == 1 ? 0 : vol.V, warped, z, sigma_m, s, C, vol, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_lcc_map_bwd(const float* fhat, int Cf, const float* z, const float* sigma_m, const float* g_z, float* g_warped,
                    int s, int C, int D, int H, int W, void* stream) {
    if (!fhat || !z || !sigma_m || !g_z || !g_warped || !dims_ok(C, D, H, W) || !broadcast_ok(Cf, C))
        return fail("irs_lcc_map_bwd: bad arguments");
    if (!lcc_ok(s, D, H, W)) return fail("irs_lcc_map_bwd: LCC half width must be 1 or 2 and smaller than half the volume");
    const Vol vol = make_vol(D, H, W);
    for (int c = 0; c < C; ++c)
        launch_data_bwd(IRS_DATA_GMM_LCC, fhat + (Cf == 1 ? 0 : (int64_t)c * vol.V), 0, z + (int64_t)c * vol.V,
                        sigma_m + (int64_t)c * vol.V, nullptr, 0, g_z + (int64_t)c * vol.V, nullptr, c,
                        g_warped + (int64_t)c * vol.V, nullptr, s, 1, vol, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// the window of the LNCC data term (lncc_kernels.hip): radius 1 .. IRS_MAX_HALF_WIDTH, every dim at least the window
static bool lncc_window_ok(const char* who, int radius, int D, int H, int W) {
    if (radius < 1 || radius > IRS_MAX_HALF_WIDTH) return !fail("%s: LNCC radius = %d, 1..%d", who, radius, IRS_MAX_HALF_WIDTH);
    const int n = 2 * radius + 1;
    return (D >= n && H >= n && W >= n) || !fail("%s: dims (%d, %d, %d), every one >= 2 radius + 1 = %d needed", who, D, H, W, n);
}

int irs_lncc_fwd(const float* fixed, int Cf, const float* moving, const float* upstream, int Cu, int radius, float eps, float* d,
                 float* coef, double* sums, double* partials, int C, int D, int H, int W, void* stream) {
    if (!fixed || !moving || !dims_ok(C, D, H, W) || (sums && !partials)) return fail("irs_lncc_fwd: bad arguments");
    if (!chains_ok("irs_lncc_fwd", C) || !lncc_window_ok("irs_lncc_fwd", radius, D, H, W)) return 1;
    if (!broadcast_ok(Cf, C)) return fail("irs_lncc_fwd: fixed image of %d chains, 1 or %d needed", Cf, C);
    if (upstream && !broadcast_ok(Cu, C)) return fail("irs_lncc_fwd: upstream of %d chains, 1 or %d needed", Cu, C);
    if (!positive_finite(eps)) return fail("irs_lncc_fwd: eps = %g, a finite value > 0 needed", (double)eps);
    const int64_t V = (int64_t)D * H * W;
    const LnccGeom g = lncc_geometry(D, H, W, radius);
    launch_lncc_fwd(fixed, Cf == 1 ? 0 : V, moving, upstream, Cu == 1 ? 0 : V, nullptr, 0, radius, eps, 1.0, d, coef,
                    sums ? partials : nullptr, C, g, (hipStream_t)stream);
    if (sums) launch_reduce_partials(partials, g.blocks, C, sums, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_lncc_bwd(const float* fixed, int Cf, const float* moving, const float* coef, int radius, float* g_moving, int C, int D,
                 int H, int W, void* stream) {
    if (!fixed || !moving || !coef || !g_moving || g_moving == fixed || g_moving == moving || g_moving == coef || !dims_ok(C, D, H, W))
        return fail("irs_lncc_bwd: bad arguments");
    if (!chains_ok("irs_lncc_bwd", C) || !lncc_window_ok("irs_lncc_bwd", radius, D, H, W)) return 1;
    if (!broadcast_ok(Cf, C)) return fail("irs_lncc_bwd: fixed image of %d chains, 1 or %d needed", Cf, C);
    const int64_t V = (int64_t)D * H * W;
    launch_lncc_bwd(fixed, Cf == 1 ? 0 : V, moving, coef, radius, 1.0f, g_moving, C, lncc_geometry(D, H, W, radius),
                    (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// the NGF data term (ngf_kernels.hip)
int irs_ngf_fwd(const float* fixed, int Cf, const float* moving, const float* upstream, int Cu, float eps_f, float eps_m, float* d,
                float* coef, double* sums, double* partials, int C, int D, int H, int W, void* stream) {
    if (!fixed || !moving || !dims_ok(C, D, H, W) || (sums && !partials)) return fail("irs_ngf_fwd: bad arguments");
    if (!chains_ok("irs_ngf_fwd", C)) return 1;
    if (!broadcast_ok(Cf, C)) return fail("irs_ngf_fwd: fixed image of %d chains, 1 or %d needed", Cf, C);
    if (upstream && !broadcast_ok(Cu, C)) return fail("irs_ngf_fwd: upstream of %d chains, 1 or %d needed", Cu, C);
    if (!positive_finite(eps_f) || !positive_finite(eps_m))
        return fail("irs_ngf_fwd: eps_f = %g, eps_m = %g, finite values > 0 needed", (double)eps_f, (double)eps_m);
    if ((d && (d == fixed || d == moving || d == upstream)) || (coef && (coef == fixed || coef == moving || coef == upstream || coef == d)))
        return fail("irs_ngf_fwd: an output must not be an input or the other output");
    const int64_t V = (int64_t)D * H * W;
    const LnccGeom g = lncc_geometry(D, H, W, 1);
    launch_ngf_fwd(fixed, Cf == 1 ? 0 : V, moving, upstream, Cu == 1 ? 0 : V, nullptr, 0, eps_f, eps_m, 1.0, false, d, coef,
                   sums ? partials : nullptr, C, g, (hipStream_t)stream);
    if (sums) launch_reduce_partials(partials, g.blocks, C, sums, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_ngf_bwd(const float* coef, float* g_moving, int C, int D, int H, int W, void* stream) {
    if (!coef || !g_moving || g_moving == coef || !dims_ok(C, D, H, W)) return fail("irs_ngf_bwd: bad arguments");
    if (!chains_ok("irs_ngf_bwd", C)) return 1;
    launch_ngf_bwd(coef, 1.0f, g_moving, C, lncc_geometry(D, H, W, 1), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// the mutual-information data term (mi_kernels.hip)
static bool mi_chains_ok(const char* who, int Cf, const uint8_t* mask, int Cm, int C) {
    if (!chains_ok(who, C)) return false;
    if (!broadcast_ok(Cf, C)) return !fail("%s: fixed image of %d chains, 1 or %d needed", who, Cf, C);
    return !mask || broadcast_ok(Cm, C) || !fail("%s: mask of %d chains, 1 or %d needed", who, Cm, C);
}

int irs_mi_fwd(const float* fixed, int Cf, const float* moving, const uint8_t* mask, int Cm, int bins, float f_lo, float f_hi,
               float m_lo, float m_hi, uint64_t* hist, float* table, double* stats, void* scratch, int C, int D, int H, int W,
               void* stream) {
    if (!fixed || !moving || !table || !stats || !scratch || !dims_ok(C, D, H, W)) return fail("irs_mi_fwd: bad arguments");
    if (!mi_chains_ok("irs_mi_fwd", Cf, mask, Cm, C)) return 1;
    MiBins bn;
    if (!mi_bins_ok("irs_mi_fwd", bins, f_lo, f_hi, m_lo, m_hi, bn)) return 1;
    if ((uintptr_t)scratch & 15) return fail("irs_mi_fwd: the scratch must be 16-byte aligned");
    const int64_t V = (int64_t)D * H * W;
    const size_t hist_bytes = (size_t)C * bins * bins * sizeof(uint64_t);  // (a multiple of 16)
    unsigned long long* h = hist ? (unsigned long long*)hist : (unsigned long long*)scratch;
    long long* ipart = (long long*)((char*)scratch + (hist ? 0 : hist_bytes));
    HIP_TRY(launch_mi_fwd(fixed, Cf == 1 ? 0 : V, moving, mask, mask && Cm != 1 ? V : 0, V, C, bn, h, table, stats, ipart, 1.0, nullptr, 0,
                          (hipStream_t)stream));
    LAUNCH_CHECK();
    return 0;
}

int irs_mi_bwd(const float* fixed, int Cf, const float* moving, const uint8_t* mask, int Cm, const float* table, int bins, float f_lo,
               float f_hi, float m_lo, float m_hi, const float* scale, float* g_moving, float* pmi, int C, int D, int H, int W,
               void* stream) {
    if (!fixed || !moving || !table || !g_moving || g_moving == fixed || g_moving == moving || g_moving == table || g_moving == pmi ||
        (pmi && (pmi == fixed || pmi == moving || pmi == table)) || !dims_ok(C, D, H, W))
        return fail("irs_mi_bwd: bad arguments");
    if (!mi_chains_ok("irs_mi_bwd", Cf, mask, Cm, C)) return 1;
    MiBins bn;
    if (!mi_bins_ok("irs_mi_bwd", bins, f_lo, f_hi, m_lo, m_hi, bn)) return 1;
    const int64_t V = (int64_t)D * H * W;
    launch_mi_bwd(fixed, Cf == 1 ? 0 : V, moving, mask, mask && Cm != 1 ? V : 0, table, V, C, bn, 1.0f, scale, false, g_moving, pmi,
                  (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_reg_energy(const float* v, double* y_out, double* partials, int C, int D, int H, int W, void* stream) {
    if (!v || !y_out || !partials || !dims_ok(C, D, H, W) || !chain_count_ok(C)) return fail("irs_reg_energy: bad arguments");
    const Vol vol = make_vol(D, H, W);
    launch_reg_energy(v, partials, C, vol, (hipStream_t)stream);
    launch_reduce_partials(partials, energy_blocks(vol), C, y_out, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_bending_energy(const float* v, double* y_out, double* partials, int C, int D, int H, int W, void* stream) {
    if (!v || !y_out || !partials || !dims_ok(C, D, H, W) || !chain_count_ok(C)) return fail("irs_bending_energy: bad arguments");
    const Vol vol = make_vol(D, H, W);
    launch_bending_energy(v, partials, energy_blocks(vol), C, vol, (hipStream_t)stream);
    launch_reduce_partials(partials, energy_blocks(vol), C, y_out, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_bending_energy_grad(const float* v, const float* scale, float* out, int C, int D, int H, int W, void* stream) {
    if (!v || !out || v == out || !dims_ok(C, D, H, W) || !chain_count_ok(C)) return fail("irs_bending_energy_grad: bad arguments");
    launch_bending_grad(v, scale, out, C, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_gradient_operator(const float* v, float* nabla, int transformation, int C, int D, int H, int W, void* stream) {
    if (!v || !nabla || !dims_ok(C, D, H, W)) return fail("irs_gradient_operator: bad arguments");
    launch_gradient_operator(v, nabla, transformation, C, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_log_det_jacobian(const float* transformation, float* log_det, long long* nan_count, int C, int D, int H, int W,
                         void* stream) {
    if (!transformation || !nan_count || !dims_ok(C, D, H, W)) return fail("irs_log_det_jacobian: bad arguments");
    launch_log_det_jacobian(transformation, log_det, nan_count, C, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// average surface distance (metric_kernels.hip)
// ================================================================================================
constexpr size_t kSurfScratchBudget = (size_t)256 << 20;  // envelope slots of lines longer than kSurfLdsLine
constexpr int kSurfMaxSlots = 4096;

static size_t surf_align(size_t x) { return (x + 255) & ~(size_t)255; }

// the per-pair table, the workspace layout and the launch shapes, from the host copy of the boxes
struct SurfLayout {
    std::vector<SurfPair> plan;
    int64_t tasks[3] = {0, 0, 0};
    int line[3] = {0, 0, 0};
    int lanes = 1;
    int slots[3] = {0, 0, 0};
    size_t plan_off = 0, partials_off = 0, memb_off = 0, ga_off = 0, gb_off = 0, env_off[3] = {0, 0, 0}, bytes = 0;
};

// the volume of a call on label maps alone: dims of at least 1 (a map may be one row of voxels), < 2^30 voxels
static bool label_dims_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && (int64_t)D * H * W < ((int64_t)1 << 30); }

// thin: dims of 1 are taken (the surface posterior; the distance calls keep the rule of the transition, dims of at least 2)
static int surface_layout(const int32_t* boxes, int P, int D, int H, int W, SurfLayout* out, bool thin = false) {
    if (!boxes || P < 1 || !(thin ? label_dims_ok(D, H, W) : dims_ok(1, D, H, W))) return fail("irs_surface_distance: bad boxes / dims");
    SurfLayout& s = *out;
    s.plan.assign((size_t)P + 1, SurfPair{});
    const int dims[3] = {D, H, W};
    int64_t vox = 0;
    int nx_max = 1;
    for (int p = 0; p < P; ++p) {
        const int32_t* b = boxes + 6 * (int64_t)p;
        SurfPair& q = s.plan[p];
        q.vox = vox;
        q.tw = s.tasks[0];
        q.th = s.tasks[1];
        q.td = s.tasks[2];
        if (b[0] > b[3]) continue;  // label in neither map
        for (int a = 0; a < 3; ++a)
            if (b[a] < 0 || b[a] > b[3 + a] || b[3 + a] >= dims[a]) return fail("irs_surface_distance: box %d out of the volume", p);
        q.z0 = b[0], q.y0 = b[1], q.x0 = b[2];
        q.nz = b[3] - b[0] + 1, q.ny = b[4] - b[1] + 1, q.nx = b[5] - b[2] + 1;
        const int chunks = (q.nx + kWave - 1) / kWave;
        vox += (int64_t)q.nz * q.ny * q.nx;
        s.tasks[0] += (int64_t)q.nz * q.ny;
        s.tasks[1] += (int64_t)q.nz * chunks;
        s.tasks[2] += (int64_t)q.ny * chunks;
        s.line[1] = std::max(s.line[1], q.ny);
        s.line[2] = std::max(s.line[2], q.nz);
        nx_max = std::max(nx_max, q.nx);
    }
    SurfPair& end = s.plan[P];
    end.vox = vox;
    end.tw = s.tasks[0];
    end.th = s.tasks[1];
    end.td = s.tasks[2];
    s.lanes = std::min(nx_max, kWave);  // a lane at or above nx_max never holds an envelope
    size_t off = surf_align(sizeof(SurfPair) * s.plan.size());
    s.partials_off = off;
    off = surf_align(off + sizeof(double) * 4 * (size_t)s.tasks[2]);
    s.memb_off = off;
    off = surf_align(off + (size_t)vox);
    s.ga_off = off;
    off = surf_align(off + sizeof(float) * (size_t)vox);
    s.gb_off = off;
    off = surf_align(off + sizeof(float) * (size_t)vox);
    for (int pass = 1; pass <= 2; ++pass) {
        if (s.line[pass] <= kSurfLdsLine || s.tasks[pass] == 0) continue;
        const size_t slot = sizeof(float) * 3 * (size_t)s.line[pass] * s.lanes;
        s.slots[pass] = (int)std::max<int64_t>(1, std::min<int64_t>({s.tasks[pass], (int64_t)(kSurfScratchBudget / slot), kSurfMaxSlots}));
        s.env_off[pass] = off;
        off = surf_align(off + slot * s.slots[pass]);
    }
    s.bytes = off;
    return 0;
}

static bool labels_ok(const char* who, const int32_t* labels, int n) {
    bool ok = labels && n >= 1 && n <= IRS_MAX_LABELS;
    for (int i = 0; ok && i < n; ++i) ok = labels[i] >= INT16_MIN && labels[i] <= INT16_MAX;
    return ok || !fail("%s: 1..%d labels in the int16 range", who, IRS_MAX_LABELS);
}

// 1 .. IRS_MAX_LABELS distinct labels in the int16 range
static bool distinct_labels_ok(const char* who, const int32_t* labels, int K) {
    if (!labels_ok(who, labels, K)) return false;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < i; ++j)
            if (labels[i] == labels[j]) return !fail("%s: label %d appears twice", who, labels[i]);
    return true;
}

static SurfLabels surf_labels(const int32_t* labels, int n) {
    SurfLabels lab = {};
    memcpy(lab.v, labels, sizeof(int32_t) * n);
    return lab;
}

// what irs_label_surface_distance and irs_label_hausdorff_distance ask of their host arrays alike
static bool surf_arrays_ok(const char* who, const int32_t* labels, int n_labels, const float* spacing) {
    if (!labels_ok(who, labels, n_labels)) return false;
    for (int a = 0; a < 3; ++a)
        if (!positive_finite(spacing[a])) return !fail("%s: spacing must be positive", who);
    return true;
}

// the table is small; the copy is waited for so that the host vector may go (its source is pageable memory)
static int upload_plan(uint8_t* ws, const SurfLayout& s, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(ws, s.plan.data(), sizeof(SurfPair) * s.plan.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the passes' views of a workspace laid out by surface_layout (the table uploaded at its head)
static SurfPassArgs surf_pass_args(uint8_t* ws, const SurfLayout& s) {
    SurfPassArgs a = {};
    a.plan = (const SurfPair*)ws;
    a.P = (int)s.plan.size() - 1;
    for (int pass = 0; pass < 3; ++pass) {
        a.tasks[pass] = s.tasks[pass];
        a.line[pass] = s.line[pass];
        a.env_scratch[pass] = s.slots[pass] ? (float*)(ws + s.env_off[pass]) : nullptr;
        a.env_slots[pass] = s.slots[pass];
    }
    a.lanes = s.lanes;
    a.memb = ws + s.memb_off;
    a.gA = (float*)(ws + s.ga_off);
    a.gB = (float*)(ws + s.gb_off);
    a.partials = (double*)(ws + s.partials_off);
    return a;
}

int irs_label_boxes(const int16_t* seg_fixed, int Cf, const int16_t* seg_moving, const int32_t* labels, int n_labels,
                    int32_t* boxes, int C, int D, int H, int W, void* stream) {
    if (!seg_fixed || !seg_moving || !boxes || !label_dims_ok(D, H, W) || !chain_count_ok(C) || !broadcast_ok(Cf, C))
        return fail("irs_label_boxes: bad arguments");
    if (!labels_ok(__func__, labels, n_labels)) return 1;
    const Vol vol = make_vol(D, H, W);
    launch_surface_boxes(seg_fixed, Cf == 1 ? 0 : vol.V, seg_moving, surf_labels(labels, n_labels), n_labels, boxes, C, vol,
                         (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_surface_distance_workspace(const int32_t* boxes, int n_pairs, int D, int H, int W, size_t* bytes) {
    if (!bytes) return fail("irs_surface_distance_workspace: null argument");
    SurfLayout s;
    if (surface_layout(boxes, n_pairs, D, H, W, &s)) return 1;
    *bytes = s.bytes;
    return 0;
}

int irs_label_surface_distance(const int16_t* seg_fixed, int Cf, const int16_t* seg_moving, const int32_t* labels,
                               int n_labels, const float* spacing, const int32_t* boxes, void* workspace,
                               size_t workspace_bytes, long long* counts, double* sums, int C, int D, int H, int W,
                               void* stream) {
    if (!seg_fixed || !seg_moving || !spacing || !workspace || !counts || !sums || !dims_ok(C, D, H, W) || !chain_count_ok(C) ||
        !broadcast_ok(Cf, C))
        return fail("irs_label_surface_distance: bad arguments");
    if (!surf_arrays_ok(__func__, labels, n_labels, spacing)) return 1;
    SurfLayout s;
    if (surface_layout(boxes, C * n_labels, D, H, W, &s)) return 1;
    if (!workspace_ok(__func__, workspace_bytes, s.bytes, "irs_surface_distance_workspace")) return 1;
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    if (upload_plan(ws, s, st)) return 1;
    const Vol vol = make_vol(D, H, W);
    launch_surface_distance(seg_fixed, Cf == 1 ? 0 : vol.V, seg_moving, surf_labels(labels, n_labels), n_labels, spacing,
                            surf_pass_args(ws, s), counts, sums, vol, st);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// Hausdorff and percentile surface distances (metric_kernels.hip pass D with KEEP + hausdorff_kernels.hip)
// ================================================================================================
constexpr int64_t kHdSliceVoxels = 65536;  // voxels of the largest box per histogram block ...
constexpr int kHdMaxSlices = 256;          // ... up to this many blocks per (pair, direction)

// the ASD workspace, then the per-task maxima, the histograms and the per-rank state of the selection
struct HdLayout {
    SurfLayout s;
    int slices = 1;
    size_t maxpart_off = 0, hist_off = 0, hist_bytes = 0, prefix_off = 0, rank_off = 0, bytes = 0;
};

static int hausdorff_layout(const int32_t* boxes, int P, int Q, int D, int H, int W, HdLayout* out, bool thin = false) {
    if (Q < 0 || Q > IRS_HAUSDORFF_MAX_PERCENTILES)
        return fail("irs_label_hausdorff_distance: 0..%d percentiles, got %d", IRS_HAUSDORFF_MAX_PERCENTILES, Q);
    HdLayout& h = *out;
    if (surface_layout(boxes, P, D, H, W, &h.s, thin)) return 1;
    int64_t largest = 1;
    for (int p = 0; p < P; ++p) largest = std::max(largest, h.s.plan[p + 1].vox - h.s.plan[p].vox);
    h.slices = (int)std::min<int64_t>((largest + kHdSliceVoxels - 1) / kHdSliceVoxels, kHdMaxSlices);
    size_t off = h.s.bytes;
    h.maxpart_off = off;
    off = surf_align(off + sizeof(uint32_t) * 2 * (size_t)h.s.tasks[2]);
    h.hist_off = off;
    h.hist_bytes = sizeof(uint32_t) * 256 * 4 * 2 * (size_t)P * Q;
    off = surf_align(off + h.hist_bytes);
    h.prefix_off = off;
    off = surf_align(off + sizeof(uint32_t) * 2 * (size_t)P * Q);
    h.rank_off = off;
    off = surf_align(off + sizeof(long long) * 2 * (size_t)P * Q);
    h.bytes = off;
    return 0;
}

int irs_hausdorff_workspace(const int32_t* boxes, int n_pairs, int Q, int D, int H, int W, size_t* bytes) {
    if (!bytes) return fail("irs_hausdorff_workspace: null argument");
    HdLayout h;
    if (hausdorff_layout(boxes, n_pairs, Q, D, H, W, &h)) return 1;
    *bytes = h.bytes;
    return 0;
}

int irs_label_hausdorff_distance(const int16_t* seg_fixed, int Cf, const int16_t* seg_moving, const int32_t* labels,
                                 int n_labels, const float* spacing, const int32_t* boxes, void* workspace,
                                 size_t workspace_bytes, const double* percentiles, int Q, long long* counts, double* sums,
                                 double* hd, double* hd_pct, int C, int D, int H, int W, void* stream) {
    if (!seg_fixed || !seg_moving || !spacing || !workspace || !counts || !sums || !hd || !dims_ok(C, D, H, W) ||
        !chain_count_ok(C) || !broadcast_ok(Cf, C))
        return fail("irs_label_hausdorff_distance: bad arguments");
    if (!surf_arrays_ok(__func__, labels, n_labels, spacing)) return 1;
    HdLayout h;
    if (hausdorff_layout(boxes, C * n_labels, Q, D, H, W, &h)) return 1;
    if (Q > 0 && (!percentiles || !hd_pct)) return fail("irs_label_hausdorff_distance: %d percentiles need percentiles and hd_pct", Q);
    for (int r = 0; r < Q; ++r)
        if (!(percentiles[r] > 0.0) || !(percentiles[r] <= 100.0) || (r > 0 && !(percentiles[r] > percentiles[r - 1])))
            return fail("irs_label_hausdorff_distance: percentiles must lie in (0, 100] and increase strictly");
    if (!workspace_ok(__func__, workspace_bytes, h.bytes, "irs_hausdorff_workspace")) return 1;
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    if (upload_plan(ws, h.s, st)) return 1;
    if (h.hist_bytes) HIP_TRY(hipMemsetAsync(ws + h.hist_off, 0, h.hist_bytes, st));
    SurfPassArgs a = surf_pass_args(ws, h.s);
    a.maxpart = (uint32_t*)(ws + h.maxpart_off);  // pass D keeps the squared distances
    const Vol vol = make_vol(D, H, W);
    launch_surface_distance(seg_fixed, Cf == 1 ? 0 : vol.V, seg_moving, surf_labels(labels, n_labels), n_labels, spacing, a, counts,
                            sums, vol, st);
    HdArgs g = {};
    g.plan = a.plan;
    g.P = a.P;
    g.Q = Q;
    g.slices = h.slices;
    for (int r = 0; r < Q; ++r) g.pct[r] = percentiles[r];
    g.memb = a.memb;
    g.gA = a.gA;
    g.gB = a.gB;
    g.counts = counts;
    g.maxpart = a.maxpart;
    g.hist = (uint32_t*)(ws + h.hist_off);
    g.prefix = (uint32_t*)(ws + h.prefix_off);
    g.rank = (long long*)(ws + h.rank_off);
    g.hd = hd;
    g.hd_pct = hd_pct;
    launch_hausdorff_select(g, st);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// surface posterior (metric_kernels.hip pass D with KEEP + surface_kernels.hip)
// ================================================================================================
int irs_surface_posterior_workspace(const int32_t* boxes, int n_pairs, int D, int H, int W, size_t* bytes) {
    if (!bytes) return fail("irs_surface_posterior_workspace: null argument");
    HdLayout h;
    if (hausdorff_layout(boxes, n_pairs, 0, D, H, W, &h, true)) return 1;
    *bytes = h.bytes;
    return 0;
}

int irs_surface_posterior_update(const int16_t* seg_fixed, const int16_t* seg_moving, const int32_t* labels, int n_labels,
                                 const float* spacing, const int32_t* boxes, void* workspace, size_t workspace_bytes, float* mean,
                                 float* m2, int32_t* count, int C, int D, int H, int W, void* stream) {
    if (!seg_fixed || !seg_moving || !spacing || !workspace || !mean || !m2 || !count || !label_dims_ok(D, H, W))
        return fail("irs_surface_posterior_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!distinct_labels_ok(__func__, labels, n_labels)) return 1;
    if (!positive3(__func__, "spacing", spacing)) return 1;
    HdLayout h;
    if (hausdorff_layout(boxes, C * n_labels, 0, D, H, W, &h, true)) return 1;
    if (!workspace_ok(__func__, workspace_bytes, h.bytes, "irs_surface_posterior_workspace")) return 1;
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    if (upload_plan(ws, h.s, st)) return 1;
    SurfPassArgs a = surf_pass_args(ws, h.s);
    a.maxpart = (uint32_t*)(ws + h.maxpart_off);  // pass D keeps the squared distances
    const Vol vol = make_vol(D, H, W);
    const SurfLabels lab = surf_labels(labels, n_labels);
    launch_surface_distance(seg_fixed, 0, seg_moving, lab, n_labels, spacing, a, nullptr, nullptr, vol, st);
    launch_surface_posterior_update(seg_fixed, seg_moving, lab, n_labels, a.plan, a.gB, C, mean, m2, count, vol, st);
    LAUNCH_CHECK();
    return 0;
}

int irs_surface_posterior_finalize(const int16_t* seg_fixed, const int32_t* labels, int n_labels, const float* mean, const float* m2,
                                   const int32_t* count, const uint8_t* mask, const double* z, int n_levels, float* bias, float* std,
                                   long long* isummary, double* fsummary, void* ws, size_t ws_bytes, int D, int H, int W,
                                   void* stream) {
    if (!seg_fixed || !mean || !m2 || !count || !bias || !std || !isummary || !fsummary || !ws || !label_dims_ok(D, H, W))
        return fail("irs_surface_posterior_finalize: bad arguments");
    if (!distinct_labels_ok(__func__, labels, n_labels)) return 1;
    if (n_levels < 0 || n_levels > IRS_SURFACE_MAX_LEVELS || (n_levels > 0 && !z))
        return fail("irs_surface_posterior_finalize: 0..%d coverage levels with their z, got %d", IRS_SURFACE_MAX_LEVELS, n_levels);
    SurfLevels lv = {};
    lv.n = n_levels;
    for (int q = 0; q < n_levels; ++q) {
        if (!(z[q] > 0.0) || !isfinite(z[q])) return fail("irs_surface_posterior_finalize: z[%d] = %g, a finite value > 0 needed", q, z[q]);
        lv.z[q] = z[q];
    }
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_SURFACE_WS_BYTES, "IRS_SURFACE_WS_BYTES")) return 1;
    launch_surface_posterior_finalize(seg_fixed, surf_labels(labels, n_labels), n_labels, mean, m2, count, mask, lv, bias, std,
                                      isummary, fsummary, ws, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// split-R-hat over chains (diag_kernels.hip)
// ================================================================================================
int irs_chain_moments_update(const float* x, int C, int D, int H, int W, int half, int k, float* mean, float* m2, void* stream) {
    if (!x || !mean || !m2 || !dims_ok(C, D, H, W)) return fail("irs_chain_moments_update: bad arguments");
    if (half != 0 && half != 1) return fail("irs_chain_moments_update: half must be 0 or 1, got %d", half);
    if (k < 1) return fail("irs_chain_moments_update: k must be >= 1, got %d", k);
    const int64_t n = (int64_t)C * 3 * D * H * W;
    launch_chain_moments(x, mean + half * n, m2 + half * n, n, k, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_split_rhat_workspace(int C, int D, int H, int W, size_t* bytes) {
    if (!bytes || !dims_ok(C, D, H, W)) return fail("irs_split_rhat_workspace: bad arguments");
    *bytes = sizeof(double) * 5 * (size_t)split_rhat_blocks((int64_t)D * H * W);
    return 0;
}

int irs_split_rhat(const float* mean, const float* m2, int C, int n, const uint8_t* mask, float thr0, float thr1, float* rhat,
                   double* summary, void* ws, size_t ws_bytes, int D, int H, int W, void* stream) {
    if (!mean || !m2 || !rhat || !summary || !ws || !dims_ok(C, D, H, W)) return fail("irs_split_rhat: bad arguments");
    if (n < 2) return fail("irs_split_rhat: n = %d samples per half chain, at least 2 needed", n);
    const int64_t V = (int64_t)D * H * W;
    const size_t need = sizeof(double) * 5 * (size_t)split_rhat_blocks(V);
    if (!workspace_ok(__func__, ws_bytes, need, "irs_split_rhat_workspace")) return 1;
    launch_split_rhat(mean, m2, C, n, mask, thr0, thr1, rhat, summary, (double*)ws, V, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// split ESS and MCSE over chains (diag_kernels.hip)
// ================================================================================================
int irs_chain_variogram_update(const float* x, int C, int D, int H, int W, int k, int L, float* ring, float* vsum, void* stream) {
    if (!x || !ring || !vsum || !dims_ok(C, D, H, W)) return fail("irs_chain_variogram_update: bad arguments");
    if (C > IRS_MAX_CHAINS) return fail("irs_chain_variogram_update: %d chains, at most %d", C, IRS_MAX_CHAINS);
    if (k < 1) return fail("irs_chain_variogram_update: k must be >= 1, got %d", k);
    if (L < 1) return fail("irs_chain_variogram_update: L must be >= 1, got %d", L);
    launch_chain_variogram(x, ring, vsum, C, (int64_t)3 * D * H * W, L, k, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_split_ess_workspace(int C, int D, int H, int W, size_t* bytes) {
    if (!bytes || !dims_ok(C, D, H, W)) return fail("irs_split_ess_workspace: bad arguments");
    *bytes = sizeof(double) * 5 * (size_t)split_rhat_blocks((int64_t)D * H * W);
    return 0;
}

int irs_split_ess(const float* mean, const float* m2, const float* vsum, int C, int n, int L, const uint8_t* mask, float threshold,
                  float* ess, float* mcse, double* summary, void* ws, size_t ws_bytes, int D, int H, int W, void* stream) {
    if (!mean || !m2 || !vsum || !ess || !mcse || !summary || !ws || !dims_ok(C, D, H, W))
        return fail("irs_split_ess: bad arguments");
    if (L < 1) return fail("irs_split_ess: L must be >= 1, got %d", L);
    if (n - 1 < 3)
        return fail("irs_split_ess: n = %d samples per half chain, at least 4 needed (the truncation rule reads lags 1 to 3)", n);
    const int64_t V = (int64_t)D * H * W;
    const size_t need = sizeof(double) * 5 * (size_t)split_rhat_blocks(V);
    if (!workspace_ok(__func__, ws_bytes, need, "irs_split_ess_workspace")) return 1;
    launch_split_ess(mean, m2, vsum, C, n, L, mask, threshold, ess, mcse, summary, (double*)ws, V, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// posterior label maps (label_kernels.hip)
// ================================================================================================

static size_t label_update_ws(int C, int K, int64_t V) { return sizeof(int32_t) * (size_t)C * K * label_update_partials_blocks(V); }

static size_t label_finalize_ws(int K, int64_t V) {
    return (sizeof(long long) * (size_t)K * (6 + 3 * IRS_LABEL_BINS) + 4 * sizeof(double)) * label_finalize_blocks(V);
}

int irs_label_posterior_workspace(int C, int K, int D, int H, int W, size_t* bytes) {
    if (!bytes || !chain_count_ok(C) || K < 1 || K > IRS_MAX_LABELS || !label_dims_ok(D, H, W))
        return fail("irs_label_posterior_workspace: bad arguments");
    const int64_t V = (int64_t)D * H * W;
    *bytes = std::max(label_update_ws(C, K, V), label_finalize_ws(K, V));
    return 0;
}

int irs_label_posterior_update(const int16_t* seg, int C, int D, int H, int W, const int32_t* labels, int K, int32_t* counts,
                               double* volume, int records_before, void* ws, size_t ws_bytes, void* stream) {
    if (!seg || !counts || !volume || !ws || !label_dims_ok(D, H, W)) return fail("irs_label_posterior_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 record count")) return 1;
    if (!distinct_labels_ok(__func__, labels, K)) return 1;
    const int64_t V = (int64_t)D * H * W;
    const size_t need = label_update_ws(C, K, V);
    if (!workspace_ok(__func__, ws_bytes, need, "irs_label_posterior_workspace")) return 1;
    launch_label_update(seg, C, V, surf_labels(labels, K), K, counts, volume, records_before, (int32_t*)ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_label_posterior_finalize(const int32_t* counts, int K, int D, int H, int W, int n, const int32_t* labels,
                                 const int16_t* seg_fixed, const uint8_t* mask, float* entropy, int16_t* map_label,
                                 long long* summary, double* mask_summary, void* ws, size_t ws_bytes, void* stream) {
    if (!counts || !seg_fixed || !entropy || !map_label || !summary || !mask_summary || !ws || !label_dims_ok(D, H, W))
        return fail("irs_label_posterior_finalize: bad arguments");
    if (n < 1) return fail("irs_label_posterior_finalize: n = %d records, at least 1 needed", n);
    if (!distinct_labels_ok(__func__, labels, K)) return 1;
    const int64_t V = (int64_t)D * H * W;
    const size_t need = label_finalize_ws(K, V);
    if (!workspace_ok(__func__, ws_bytes, need, "irs_label_posterior_workspace")) return 1;
    const int blocks = label_finalize_blocks(V);
    long long* partials = (long long*)ws;
    double* dpartials = (double*)(partials + (size_t)K * (6 + 3 * IRS_LABEL_BINS) * blocks);
    launch_label_finalize(counts, K, V, n, surf_labels(labels, K), seg_fixed, mask, entropy, map_label, summary, mask_summary, partials,
                          dpartials, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// Jacobian posterior maps (jacobian_kernels.hip)
// ================================================================================================
int irs_jacobian_posterior_update(const float* transformation, int C, int D, int H, int W, int32_t* folds, float* mean, float* m2,
                                  int records_before, void* stream) {
    if (!transformation || !folds || !mean || !m2 || !dims_ok(C, D, H, W)) return fail("irs_jacobian_posterior_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 fold count")) return 1;
    launch_jacobian_update(transformation, C, folds, mean, m2, records_before, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_jacobian_posterior_finalize(const int32_t* folds, const float* mean, const float* m2, int D, int H, int W, int n,
                                    const uint8_t* mask, float* fold_prob, float* logJ_mean, float* logJ_std, long long* isummary,
                                    double* fsummary, void* ws, size_t ws_bytes, void* stream) {
    if (!folds || !mean || !m2 || !fold_prob || !logJ_mean || !logJ_std || !isummary || !fsummary || !ws || !dims_ok(1, D, H, W))
        return fail("irs_jacobian_posterior_finalize: bad arguments");
    if (n < 1) return fail("irs_jacobian_posterior_finalize: n = %d records, at least 1 needed", n);
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_JACOBIAN_WS_BYTES, "IRS_JACOBIAN_WS_BYTES")) return 1;
    launch_jacobian_finalize(folds, mean, m2, (int64_t)D * H * W, n, mask, fold_prob, logJ_mean, logJ_std, isummary, fsummary, ws,
                             (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// structure report (structure_kernels.hip)
// ================================================================================================
int irs_structure_workspace(int D, int H, int W, int n_labels, int rows, size_t* bytes) {
    if (!bytes) return fail("irs_structure_workspace: bad arguments");
    if (!structure_shape_ok(__func__, D, H, W, 1, n_labels)) return 1;
    if (rows < 1) return fail("irs_structure_workspace: rows = %d, at least 1 needed", rows);
    *bytes = structure_workspace_bytes((int64_t)D * H * W, n_labels, rows);
    return 0;
}

int irs_structure_motion(const float* displacement, const float* transformation, int C, int D, int H, int W, const int16_t* seg_fixed,
                         const int32_t* labels, int n_labels, const uint8_t* mask, const float* scale, long long* ints,
                         double* floats, void* ws, size_t ws_bytes, void* stream) {
    if (!displacement || !transformation || !seg_fixed || !labels || !scale || !ints || !floats || !ws)
        return fail("irs_structure_motion: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!structure_shape_ok(__func__, D, H, W, 2, n_labels)) return 1;
    if (!distinct_labels_ok(__func__, labels, n_labels)) return 1;
    if (!positive3(__func__, "scale", scale)) return 1;
    const Vol vol = make_vol(D, H, W);
    if (!workspace_ok(__func__, ws_bytes, structure_workspace_bytes(vol.V, n_labels, C), "irs_structure_workspace")) return 1;
    launch_structure_motion(displacement, transformation, seg_fixed, surf_labels(labels, n_labels), n_labels, mask, scale, ints, floats,
                            ws, C, vol, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_structure_map_stats(const float* maps, int M, int D, int H, int W, const int16_t* seg_fixed, const int32_t* labels,
                            int n_labels, const uint8_t* mask, long long* ints, double* floats, void* ws, size_t ws_bytes,
                            void* stream) {
    if (!maps || !seg_fixed || !labels || !ints || !floats || !ws) return fail("irs_structure_map_stats: bad arguments");
    if (M < 1) return fail("irs_structure_map_stats: M = %d maps, at least 1 needed", M);
    if (!structure_shape_ok(__func__, D, H, W, 1, n_labels)) return 1;
    if (!distinct_labels_ok(__func__, labels, n_labels)) return 1;
    const int64_t V = (int64_t)D * H * W;
    if (!workspace_ok(__func__, ws_bytes, structure_workspace_bytes(V, n_labels, M), "irs_structure_workspace")) return 1;
    launch_structure_map_stats(maps, M, V, seg_fixed, surf_labels(labels, n_labels), n_labels, mask, ints, floats, ws,
                               (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// known-transformation validation (truth_kernels.hip)
// ================================================================================================
int irs_truth_update(const float* displacement, int C, int D, int H, int W, const float* truth, uint16_t* below, const uint8_t* mask,
                     const float* scale, int records_before, long long* ints, double* floats, void* ws, size_t ws_bytes,
                     void* stream) {
    if (!displacement || !truth || !below || !scale || !ints || !floats || !ws || !dims_ok(C, D, H, W))
        return fail("irs_truth_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!positive3(__func__, "scale", scale)) return 1;
    if (!records_ok(__func__, records_before, C, IRS_TRUTH_MAX_RECORDS, "exceed the 65535 a uint16 count holds")) return 1;
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_TRUTH_UPDATE_WS_BYTES, "IRS_TRUTH_UPDATE_WS_BYTES")) return 1;
    launch_truth_update(displacement, C, truth, below, mask, scale, records_before, (int64_t)D * H * W, ints, floats, ws,
                        (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_truth_calibrate(const float* mean, const float* comoment, const uint16_t* below, const float* truth, int D, int H, int W, int n,
                        const float* scale, double std_floor, const uint8_t* mask, const double* d2_edges, int pit_bins,
                        const double* levels, int n_levels, int rank_bins, const double* var_edges, int reliability_bins,
                        float* error, float* mahalanobis, long long* counts, long long* rel_ints, double* rel_floats,
                        long long* isummary, double* fsummary, void* ws, size_t ws_bytes, void* stream) {
    if (!mean || !comoment || !below || !truth || !scale || !levels || !error || !mahalanobis || !counts || !rel_ints || !rel_floats ||
        !isummary || !fsummary || !ws || !dims_ok(1, D, H, W))
        return fail("irs_truth_calibrate: bad arguments");
    if (n < 2) return fail("irs_truth_calibrate: n = %d records, at least 2 needed", n);
    if (n > IRS_TRUTH_MAX_RECORDS)
        return fail("irs_truth_calibrate: n = %d records, but the uint16 counts of `below` hold at most %d", n, IRS_TRUTH_MAX_RECORDS);
    if (!positive3(__func__, "scale", scale)) return 1;
    if (!(std_floor > 0.0) || !isfinite(std_floor) || !(std_floor * std_floor > 0.0))
        return fail("irs_truth_calibrate: std_floor = %g, a finite value > 0 (whose square is > 0) needed", std_floor);
    if (!count_ok(__func__, "pit_bins", pit_bins, IRS_TRUTH_MAX_BINS) || !count_ok(__func__, "n_levels", n_levels, IRS_TRUTH_MAX_LEVELS) ||
        !count_ok(__func__, "rank_bins", rank_bins, IRS_TRUTH_MAX_BINS) ||
        !count_ok(__func__, "reliability_bins", reliability_bins, IRS_TRUTH_MAX_RELIABILITY_BINS))
        return 1;
    if ((pit_bins > 1 && !d2_edges) || (reliability_bins > 1 && !var_edges)) return fail("irs_truth_calibrate: bad arguments");
    if (!thresholds_ok(__func__, "d2_edges", d2_edges, pit_bins - 1, true) || !thresholds_ok(__func__, "levels", levels, n_levels, false) ||
        !thresholds_ok(__func__, "var_edges", var_edges, reliability_bins - 1, true))
        return 1;
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_TRUTH_CALIBRATE_WS_BYTES, "IRS_TRUTH_CALIBRATE_WS_BYTES")) return 1;
    launch_truth_calibrate(mean, comoment, below, truth, (int64_t)D * H * W, n, scale, std_floor, mask, d2_edges, pit_bins, levels,
                           n_levels, rank_bins, var_edges, reliability_bins, error, mahalanobis, counts, rel_ints, rel_floats, isummary,
                           fsummary, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// image posterior (image_posterior_kernels.hip)
// ================================================================================================
int irs_image_posterior_update(const float* volumes, int S, const float* transformation, int C, int D, int H, int W, float* mean,
                               float* m2, float* low, float* high, int records_before, void* stream) {
    if (!volumes || !transformation || !mean || !m2 || !low || !high || !dims_ok(C, D, H, W))
        return fail("irs_image_posterior_update: bad arguments");
    if (S < 1 || S > IRS_IMAGE_POSTERIOR_MAX_VOLUMES)
        return fail("irs_image_posterior_update: S = %d volumes, 1..%d", S, IRS_IMAGE_POSTERIOR_MAX_VOLUMES);
    if (!chains_ok(__func__, C)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 record count")) return 1;
    // the launch is one block row per (volume group, plane) and per four rows of a plane
    if ((int64_t)D * ((S + kImagePosteriorGroup - 1) / kImagePosteriorGroup) > 65535 || (H + 3) / 4 > 65535)
        return fail("irs_image_posterior_update: dims (%d, %d, %d) x %d volumes exceed the launch grid", D, H, W, S);
    launch_image_posterior_update(volumes, S, transformation, C, mean, m2, low, high, records_before, make_vol(D, H, W),
                                  (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_image_posterior_finalize(const float* mean, const float* m2, const float* low, const float* high, int D, int H, int W, int n,
                                 const float* reference, float std_floor, const uint8_t* mask, float* std_out, float* range_out,
                                 float* z_out, long long* isummary, double* fsummary, void* ws, size_t ws_bytes, void* stream) {
    if (!mean || !m2 || !low || !high || !std_out || !range_out || !isummary || !fsummary || !ws || !dims_ok(1, D, H, W))
        return fail("irs_image_posterior_finalize: bad arguments");
    if (n < 1) return fail("irs_image_posterior_finalize: n = %d records, at least 1 needed", n);
    if (!reference != !z_out) return fail("irs_image_posterior_finalize: reference and z_out go together, one of them is NULL");
    if (!(std_floor >= 0.0f) || !isfinite(std_floor))
        return fail("irs_image_posterior_finalize: std_floor = %g, a finite value >= 0 needed", (double)std_floor);
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_IMAGE_POSTERIOR_WS_BYTES, "IRS_IMAGE_POSTERIOR_WS_BYTES")) return 1;
    launch_image_posterior_finalize(mean, m2, low, high, (int64_t)D * H * W, n, reference, std_floor, mask, std_out, range_out, z_out,
                                    isummary, fsummary, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// displacement covariance posterior (covariance_kernels.hip)
// ================================================================================================
int irs_displacement_covariance_update(const float* displacement, int C, int D, int H, int W, float* mean, float* comoment,
                                       int records_before, void* stream) {
    if (!displacement || !mean || !comoment || !dims_ok(C, D, H, W)) return fail("irs_displacement_covariance_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 record count")) return 1;
    launch_covariance_update(displacement, C, mean, comoment, records_before, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_displacement_covariance_finalize(const float* mean, const float* comoment, int D, int H, int W, int n, const float* scale,
                                         const uint8_t* mask, float* stdev, float* direction, float* anisotropy, long long* isummary,
                                         double* fsummary, void* ws, size_t ws_bytes, void* stream) {
    if (!mean || !comoment || !scale || !stdev || !direction || !anisotropy || !isummary || !fsummary || !ws || !dims_ok(1, D, H, W))
        return fail("irs_displacement_covariance_finalize: bad arguments");
    if (n < 1) return fail("irs_displacement_covariance_finalize: n = %d records, at least 1 needed", n);
    if (!positive3(__func__, "scale", scale)) return 1;
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_COVARIANCE_WS_BYTES, "IRS_COVARIANCE_WS_BYTES")) return 1;
    launch_covariance_finalize(mean, comoment, (int64_t)D * H * W, n, scale, mask, stdev, direction, anisotropy, isummary, fsummary, ws,
                               (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// posterior comparison (compare_kernels.hip)
// ================================================================================================
int irs_posterior_compare(const float* mean_a, const float* comoment_a, int n_a, const float* mean_b, const float* comoment_b, int n_b,
                          int D, int H, int W, const float* scale, double std_floor, const uint8_t* mask, float* shift,
                          float* log_std_ratio, float* bures, float* jeffreys, long long* isummary, double* fsummary, void* ws,
                          size_t ws_bytes, void* stream) {
    if (!mean_a || !comoment_a || !mean_b || !comoment_b || !scale || !shift || !log_std_ratio || !bures || !jeffreys || !isummary ||
        !fsummary || !ws || !dims_ok(1, D, H, W))
        return fail("irs_posterior_compare: bad arguments");
    if (n_a < 2 || n_b < 2) return fail("irs_posterior_compare: n_a = %d and n_b = %d records, at least 2 each needed", n_a, n_b);
    if (!positive3(__func__, "scale", scale)) return 1;
    if (!(std_floor > 0.0) || !isfinite(std_floor) || !(std_floor * std_floor > 0.0))
        return fail("irs_posterior_compare: std_floor = %g, a finite value > 0 (whose square is > 0) needed", std_floor);
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_COMPARE_WS_BYTES, "IRS_COMPARE_WS_BYTES")) return 1;
    launch_posterior_compare(mean_a, comoment_a, n_a, mean_b, comoment_b, n_b, (int64_t)D * H * W, scale, std_floor, mask, shift,
                             log_std_ratio, bures, jeffreys, isummary, fsummary, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// displacement credible intervals (quantile_kernels.hip)
// ================================================================================================
static bool quantile_bins_ok(int bins) { return bins >= IRS_QUANTILE_MIN_BINS && bins <= IRS_QUANTILE_MAX_BINS && bins % 2 == 0; }
#define IRS_STR_(x) #x
#define IRS_STR(x) IRS_STR_(x)

int irs_displacement_quantiles_update(const float* displacement, int C, int D, int H, int W, float* centre, uint16_t* hist,
                                      int bins, const float* inv_width, int records_before, void* stream) {
    if (!displacement || !centre || !hist || !inv_width || !dims_ok(C, D, H, W))
        return fail("irs_displacement_quantiles_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!quantile_bins_ok(bins))
        return fail("irs_displacement_quantiles_update: bins = %d, an even number in %d..%d needed", bins, IRS_QUANTILE_MIN_BINS,
                    IRS_QUANTILE_MAX_BINS);
    if (!positive3(__func__, "inv_width", inv_width)) return 1;
    if (!records_ok(__func__, records_before, C, IRS_QUANTILE_MAX_RECORDS,
                    "exceed the " IRS_STR(IRS_QUANTILE_MAX_RECORDS) " a uint16 count holds"))
        return 1;
    launch_quantile_update(displacement, C, centre, hist, bins, inv_width, records_before, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_displacement_quantiles_finalize(const float* centre, const uint16_t* hist, int bins, int D, int H, int W, int n,
                                        const float* width, const float* scale, const double* probs, int P, const uint8_t* mask,
                                        float* quantiles, float* ci_width, long long* isummary, double* fsummary, void* ws,
                                        size_t ws_bytes, void* stream) {
    if (!centre || !hist || !width || !scale || !probs || !quantiles || !ci_width || !isummary || !fsummary || !ws ||
        !dims_ok(1, D, H, W))
        return fail("irs_displacement_quantiles_finalize: bad arguments");
    if (!quantile_bins_ok(bins))
        return fail("irs_displacement_quantiles_finalize: bins = %d, an even number in %d..%d needed", bins, IRS_QUANTILE_MIN_BINS,
                    IRS_QUANTILE_MAX_BINS);
    if (n < 1 || n > IRS_QUANTILE_MAX_RECORDS)
        return fail("irs_displacement_quantiles_finalize: n = %d records, 1..%d needed", n, IRS_QUANTILE_MAX_RECORDS);
    if (P < 2 || P > IRS_QUANTILE_MAX_PROBS)
        return fail("irs_displacement_quantiles_finalize: P = %d probabilities, 2..%d needed", P, IRS_QUANTILE_MAX_PROBS);
    for (int j = 0; j < P; ++j)
        if (!(probs[j] > 0.0 && probs[j] < 1.0) || (j > 0 && !(probs[j] > probs[j - 1])))
            return fail("irs_displacement_quantiles_finalize: probs[%d] = %g, strictly increasing values in (0,1) needed", j, probs[j]);
    for (int a = 0; a < 3; ++a) {
        if (!positive_finite(width[a]))
            return fail("irs_displacement_quantiles_finalize: width[%d] = %g, a finite value > 0 needed", a, (double)width[a]);
        if (!positive_finite(scale[a]))
            return fail("irs_displacement_quantiles_finalize: scale[%d] = %g, a finite value > 0 needed", a, (double)scale[a]);
    }
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_QUANTILE_WS_BYTES, "IRS_QUANTILE_WS_BYTES")) return 1;
    launch_quantile_finalize(centre, hist, bins, (int64_t)D * H * W, n, width, scale, probs, P, mask, quantiles, ci_width, isummary,
                             fsummary, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// inverse transformation and inverse-consistency error (inverse_kernels.hip)
// ================================================================================================
int irs_svf_exp_inverse(const float* v, float* scratch, float* transformation, float* displacement, int no_steps, int C, int D,
                        int H, int W, void* stream) {
    if (!v || !scratch || !dims_ok(C, D, H, W) || no_steps < 1 || no_steps > 30) return fail("irs_svf_exp_inverse: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const Vol vol = make_vol(D, H, W);
    Lin lin;
    if (cached_lin(D, H, W, st, &lin)) return fail("irs_svf_exp_inverse: identity grid allocation failed");
    const int64_t field = (int64_t)C * 3 * vol.V;
    float* buf[2] = {scratch, scratch + field};
    launch_negate(v, buf[1], field, st);
    for (int k = 0; k < no_steps; ++k)  // step 0: buf[1] -> buf[0]; then ping-pong
        launch_exp_step_fwd_march(buf[(k + 1) & 1], buf[k & 1], k == 0, no_steps, C, vol, lin, nullptr, nullptr, false, 0, st);
    if (transformation || displacement) launch_svf_outputs(buf[(no_steps - 1) & 1], transformation, displacement, C, vol, lin, st);
    LAUNCH_CHECK();
    return 0;
}

int irs_inverse_consistency(const float* t_a, const float* d_a, const float* d_b, const float* scale, const uint8_t* mask,
                            int mask_chains, float* residual, float* norm, long long* isummary, double* fsummary, void* ws,
                            size_t ws_bytes, int C, int D, int H, int W, void* stream) {
    if (!t_a || !d_a || !d_b || !scale || !isummary || !fsummary || !ws || !dims_ok(C, D, H, W))
        return fail("irs_inverse_consistency: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (mask && !broadcast_ok(mask_chains, C))
        return fail("irs_inverse_consistency: mask of %d chains, 1 or %d needed", mask_chains, C);
    if (!positive3(__func__, "scale", scale)) return 1;
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_ICE_WS_BYTES, "IRS_ICE_WS_BYTES")) return 1;
    launch_inverse_consistency(t_a, d_a, d_b, scale, mask, mask_chains, residual, norm, isummary, fsummary, ws, C, make_vol(D, H, W),
                               (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_inverse_consistency_update(const float* norm, int C, int D, int H, int W, float* mean, float* peak, int records_before,
                                   void* stream) {
    if (!norm || !mean || !peak || !dims_ok(C, D, H, W)) return fail("irs_inverse_consistency_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 record count")) return 1;
    launch_inverse_consistency_update(norm, C, (int64_t)D * H * W, mean, peak, records_before, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_inverse_consistency_finalize(const float* mean, const float* peak, int D, int H, int W, const uint8_t* mask,
                                     float threshold, long long* isummary, double* fsummary, void* ws, size_t ws_bytes,
                                     void* stream) {
    if (!mean || !peak || !isummary || !fsummary || !ws || !dims_ok(1, D, H, W))
        return fail("irs_inverse_consistency_finalize: bad arguments");
    if (!positive_finite(threshold))
        return fail("irs_inverse_consistency_finalize: threshold = %g, a finite value > 0 needed", (double)threshold);
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_ICE_MAP_WS_BYTES, "IRS_ICE_MAP_WS_BYTES")) return 1;
    launch_inverse_consistency_finalize(mean, peak, (int64_t)D * H * W, mask, threshold, isummary, fsummary, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// native-resolution outputs (native_kernels.hip)
// ================================================================================================
int irs_native_warp(const float* displacement, int C, const int32_t* dims, const int32_t* native, const int32_t* padding,
                    const float* im, const int16_t* seg, const uint8_t* mask, int Cim, float fill, const float* scale,
                    float* im_out, int16_t* seg_out, uint8_t* mask_out, float* displacement_out, void* stream) {
    if (!displacement || !dims || !native || !padding) return fail("irs_native_warp: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!broadcast_ok(Cim, C)) return fail("irs_native_warp: moving volumes of %d chains, 1 or %d needed", Cim, C);
    if (!im_out && !seg_out && !mask_out && !displacement_out) return fail("irs_native_warp: no output requested");
    if ((im_out && !im) || (seg_out && !seg) || (mask_out && !mask))
        return fail("irs_native_warp: an output is requested of a moving volume that is NULL");
    if (displacement_out && !scale) return fail("irs_native_warp: displacement_out needs scale");
    NativeGeom gm;
    int64_t voxels;
    if (!native_geometry_ok(__func__, C, dims, native, padding, 1, gm, voxels)) return 1;
    if (displacement_out)
        for (int c = 0; c < 3; ++c) {
            if (!isfinite(scale[c])) return fail("irs_native_warp: scale[%d] = %g, a finite value needed", c, (double)scale[c]);
            gm.out_scale[c] = scale[c];
        }
    if (!isfinite(fill)) return fail("irs_native_warp: fill = %g, a finite value needed", (double)fill);
    gm.fill = fill;
    launch_native_warp(displacement, im_out ? im : nullptr, seg_out ? seg : nullptr, mask_out ? mask : nullptr,
                       Cim == 1 ? 0 : voxels, im_out, seg_out, mask_out, displacement_out, gm, C, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_native_warp_cubic(const float* displacement, int C, const int32_t* dims, const int32_t* native, const int32_t* padding,
                          const float* im, const float* coeff, int Cim, float fill, float* im_out, void* stream) {
    if (!displacement || !dims || !native || !padding || !im || !coeff || !im_out) return fail("irs_native_warp_cubic: null pointer");
    if (!chains_ok(__func__, C)) return 1;
    if (!broadcast_ok(Cim, C)) return fail("irs_native_warp_cubic: moving volumes of %d chains, 1 or %d needed", Cim, C);
    NativeGeom gm;
    int64_t voxels;
    if (!native_geometry_ok(__func__, C, dims, native, padding, 2, gm, voxels)) return 1;
    if (!isfinite(fill)) return fail("irs_native_warp_cubic: fill = %g, a finite value needed", (double)fill);
    gm.fill = fill;
    launch_native_warp_cubic(displacement, im, coeff, Cim == 1 ? 0 : voxels, im_out, gm, C, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// native-grid posteriors (native_posterior_kernels.hip)
// ================================================================================================
static size_t native_posterior_ws(int C, int K, const NativeGeom& gm) {
    return sizeof(int32_t) * (size_t)C * K * native_posterior_blocks(gm);
}

int irs_native_posterior_workspace(int C, int K, const int32_t* native, size_t* bytes) {
    if (!bytes || !native || !chain_count_ok(C) || K < 0 || K > IRS_MAX_LABELS || native[0] < 2 || native[1] < 2 || native[2] < 2)
        return fail("irs_native_posterior_workspace: bad arguments");
    NativeGeom gm = {};
    for (int a = 0; a < 3; ++a) gm.n[a] = native[a];
    *bytes = std::max<size_t>(native_posterior_ws(C, K, gm), 16);  // never empty: a caller without labels still allocates it
    return 0;
}

int irs_native_posterior_update(const float* displacement, int C, const int32_t* dims, const int32_t* native, const int32_t* padding,
                                const float* im, const int16_t* seg, int Cim, float fill, const int32_t* labels, int K,
                                int32_t* counts, double* volume, float* mean, float* m2, float* low, float* high,
                                int records_before, void* ws, size_t ws_bytes, void* stream) {
    if (!displacement || !dims || !native || !padding || !ws) return fail("irs_native_posterior_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!broadcast_ok(Cim, C)) return fail("irs_native_posterior_update: moving volumes of %d chains, 1 or %d needed", Cim, C);
    const int lab_given = !!seg + !!labels + !!counts + !!volume, im_given = !!im + !!mean + !!m2 + !!low + !!high;
    if (lab_given != 0 && lab_given != 4)
        return fail("irs_native_posterior_update: seg, labels, counts and volume go together, %d of them given", lab_given);
    if (im_given != 0 && im_given != 5)
        return fail("irs_native_posterior_update: im, mean, m2, low and high go together, %d of them given", im_given);
    if (!lab_given && !im_given) return fail("irs_native_posterior_update: neither the label nor the image part is given");
    NativeGeom gm;
    int64_t voxels;
    if (!native_geometry_ok(__func__, C, dims, native, padding, 2, gm, voxels)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 record count")) return 1;
    if (lab_given && !distinct_labels_ok(__func__, labels, K)) return 1;
    if (!isfinite(fill)) return fail("irs_native_posterior_update: fill = %g, a finite value needed", (double)fill);
    gm.fill = fill;
    const size_t need = lab_given ? native_posterior_ws(C, K, gm) : 0;
    if (!workspace_ok(__func__, ws_bytes, need, "irs_native_posterior_workspace")) return 1;
    launch_native_posterior_update(displacement, im, seg, Cim == 1 ? 0 : voxels, lab_given ? surf_labels(labels, K) : SurfLabels{},
                                   lab_given ? K : 0, counts, volume, (int32_t*)ws, mean, m2, low, high, records_before, gm, C,
                                   (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// landmark propagation (landmark_kernels.hip)
// ================================================================================================
static bool landmark_count_ok(int K) { return K >= 1 && K <= IRS_LANDMARK_MAX_POINTS; }

int irs_transform_points(const float* points, int K, const float* displacement, int C, int D, int H, int W, const float* scale,
                         const float* offset, float* sampled, float* mapped, void* stream) {
    if (!points || !displacement || !scale) return fail("irs_transform_points: bad arguments");
    if (!sampled && !mapped) return fail("irs_transform_points: no output requested");
    if (!landmark_count_ok(K)) return fail("irs_transform_points: K = %d points, 1..%d", K, IRS_LANDMARK_MAX_POINTS);
    if (!chains_ok(__func__, C)) return 1;
    if (!dims_ok(C, D, H, W)) return fail("irs_transform_points: bad dims (%d, %d, %d)", D, H, W);
    if (!positive3(__func__, "scale", scale)) return 1;
    launch_transform_points(points, K, displacement, scale, offset, sampled, mapped, C, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_landmark_update(const float* mapped, const float* target, int C, int K, double* mean, double* comoment, double* tre_mean,
                        double* tre_m2, double* tre_max, int32_t* count, int records_before, void* stream) {
    if (!mapped || !target || !mean || !comoment || !tre_mean || !tre_m2 || !tre_max || !count)
        return fail("irs_landmark_update: bad arguments");
    if (!landmark_count_ok(K)) return fail("irs_landmark_update: K = %d landmarks, 1..%d", K, IRS_LANDMARK_MAX_POINTS);
    if (!chains_ok(__func__, C)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 record count")) return 1;
    launch_landmark_update(mapped, target, C, K, mean, comoment, tre_mean, tre_m2, tre_max, count, records_before, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_landmark_finalize(const double* mean, const double* comoment, const double* tre_mean, const double* tre_m2,
                          const double* tre_max, const int32_t* count, const float* target, int K, double* out, long long* isummary,
                          double* fsummary, void* ws, size_t ws_bytes, void* stream) {
    if (!mean || !comoment || !tre_mean || !tre_m2 || !tre_max || !count || !target || !out || !isummary || !fsummary || !ws)
        return fail("irs_landmark_finalize: bad arguments");
    if (!landmark_count_ok(K)) return fail("irs_landmark_finalize: K = %d landmarks, 1..%d", K, IRS_LANDMARK_MAX_POINTS);
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_LANDMARK_WS_BYTES, "IRS_LANDMARK_WS_BYTES")) return 1;
    launch_landmark_finalize(mean, comoment, tre_mean, tre_m2, tre_max, count, target, K, out, isummary, fsummary, ws,
                             (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// intensity similarity (similarity_kernels.hip)
// ================================================================================================
static size_t similarity_hist_bytes(int C, int bins) { return ((size_t)C * bins * bins * sizeof(int32_t) + 15) & ~(size_t)15; }
static size_t similarity_partials_bytes() { return (size_t)IRS_SIMILARITY_MAX_BLOCKS * (3 + 6) * 8; }

int irs_image_similarity_workspace(int C, int bins, size_t* bytes) {
    if (!bytes) return fail("irs_image_similarity_workspace: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (bins < IRS_SIMILARITY_MIN_BINS || bins > IRS_SIMILARITY_MAX_BINS)
        return fail("irs_image_similarity_workspace: bins = %d, %d..%d", bins, IRS_SIMILARITY_MIN_BINS, IRS_SIMILARITY_MAX_BINS);
    *bytes = similarity_hist_bytes(C, bins) + similarity_partials_bytes();
    return 0;
}

int irs_image_similarity(const float* fixed, int Cf, const float* moving, int C, const uint8_t* mask, int D, int H, int W,
                         float f_lo, float f_hi, float m_lo, float m_hi, int bins, int32_t* hist, double* stats, void* ws,
                         size_t ws_bytes, void* stream) {
    if (!fixed || !moving || !stats || !ws) return fail("irs_image_similarity: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!broadcast_ok(Cf, C)) return fail("irs_image_similarity: fixed image of %d chains, 1 or %d needed", Cf, C);
    if (bins < IRS_SIMILARITY_MIN_BINS || bins > IRS_SIMILARITY_MAX_BINS)
        return fail("irs_image_similarity: bins = %d, %d..%d", bins, IRS_SIMILARITY_MIN_BINS, IRS_SIMILARITY_MAX_BINS);
    if (D < 1 || H < 1 || W < 1) return fail("irs_image_similarity: dims (%d, %d, %d), every one >= 1 needed", D, H, W);
    const int64_t V = (int64_t)D * H * W;
    if (V >= ((int64_t)1 << 30)) return fail("irs_image_similarity: the volume must have fewer than 2^30 voxels");
    SimBins bn;
    bn.bins = bins;
    const float lo[2] = {f_lo, m_lo}, hi[2] = {f_hi, m_hi};
    float inv[2];
    for (int k = 0; k < 2; ++k) {
        const char* who = k == 0 ? "fixed" : "moving";
        if (!isfinite(lo[k]) || !isfinite(hi[k]) || !(hi[k] > lo[k]))
            return fail("irs_image_similarity: %s range [%g, %g], finite bounds with hi > lo needed", who, (double)lo[k], (double)hi[k]);
        const float width = hi[k] - lo[k];  // fp32, as the definition states it
        inv[k] = (float)bins / width;
        if (!isfinite(inv[k]) || !(inv[k] > 0.0f))
            return fail("irs_image_similarity: %s range [%g, %g] is too wide or too narrow for float32 bins", who, (double)lo[k], (double)hi[k]);
    }
    bn.f_lo = f_lo, bn.f_hi = f_hi, bn.f_inv = inv[0];
    bn.m_lo = m_lo, bn.m_hi = m_hi, bn.m_inv = inv[1];
    const size_t hist_bytes = similarity_hist_bytes(C, bins), need = hist_bytes + similarity_partials_bytes();
    if (!workspace_ok(__func__, ws_bytes, need, "irs_image_similarity_workspace")) return 1;
    if ((uintptr_t)ws & 15) return fail("irs_image_similarity: the workspace must be 16-byte aligned");
    long long* ipart = (long long*)((char*)ws + hist_bytes);
    double* fpart = (double*)(ipart + (size_t)IRS_SIMILARITY_MAX_BLOCKS * 3);
    launch_image_similarity(fixed, Cf == 1 ? 0 : V, moving, mask, V, C, bn, hist ? hist : (int32_t*)ws, stats, ipart, fpart,
                            (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// local similarity maps (local_similarity_kernels.hip)
// ================================================================================================

// the volume of a local-similarity call: dims of at least 1, < 2^30 voxels
static bool local_dims_ok(const char* who, int D, int H, int W) {
    if (D < 1 || H < 1 || W < 1) return !fail("%s: dims (%d, %d, %d), every one >= 1 needed", who, D, H, W);
    return (int64_t)D * H * W < ((int64_t)1 << 30) || !fail("%s: the volume must have fewer than 2^30 voxels", who);
}

int irs_local_similarity(const float* fixed, int Cf, const float* moving, int C, const uint8_t* mask, int D, int H, int W,
                         int radius, double floor_f, double floor_m, double c1, double c2, float* lncc, float* ssim,
                         double* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!fixed || !moving || !stats || !ws) return fail("irs_local_similarity: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!broadcast_ok(Cf, C)) return fail("irs_local_similarity: fixed image of %d chains, 1 or %d needed", Cf, C);
    if (radius < 1 || radius > IRS_LOCAL_MAX_RADIUS)
        return fail("irs_local_similarity: radius = %d, 1..%d", radius, IRS_LOCAL_MAX_RADIUS);
    const double values[4] = {floor_f, floor_m, c1, c2};
    const char* names[4] = {"floor_f", "floor_m", "c1", "c2"};
    for (int j = 0; j < 4; ++j)
        if (!(values[j] > 0.0) || !isfinite(values[j]))
            return fail("irs_local_similarity: %s = %g, a finite value > 0 needed", names[j], values[j]);
    if (!local_dims_ok(__func__, D, H, W)) return 1;
    const LocalGeom g = local_similarity_geometry(D, H, W, radius);
    const size_t need = (size_t)C * g.blocks * IRS_LOCAL_STATS * 8;
    if (!workspace_ok(__func__, ws_bytes, need, "IRS_LOCAL_WS_BYTES")) return 1;
    const LocalConsts k = {floor_f, floor_m, c1, c2};
    launch_local_similarity(fixed, Cf == 1 ? 0 : (int64_t)D * H * W, moving, mask, C, radius, g, k, lncc, ssim, stats, ws,
                            (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_local_similarity_update(const float* lncc, int C, int D, int H, int W, float* mean, float* low, int32_t* count,
                                int records_before, void* stream) {
    if (!lncc || !mean || !low || !count) return fail("irs_local_similarity_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (!local_dims_ok(__func__, D, H, W)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 sample count")) return 1;
    launch_local_similarity_update(lncc, C, (int64_t)D * H * W, mean, low, count, records_before, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_local_similarity_finalize(const float* mean, const float* low, const int32_t* count, const uint8_t* mask, int D, int H,
                                  int W, long long* isummary, double* fsummary, void* ws, size_t ws_bytes, void* stream) {
    if (!mean || !low || !count || !isummary || !fsummary || !ws) return fail("irs_local_similarity_finalize: bad arguments");
    if (!local_dims_ok(__func__, D, H, W)) return 1;
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_LOCAL_MAP_WS_BYTES, "IRS_LOCAL_MAP_WS_BYTES")) return 1;
    launch_local_similarity_finalize(mean, low, count, (int64_t)D * H * W, mask, isummary, fsummary, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// residual model check (residual_kernels.hip)
// ================================================================================================
int irs_residual_histogram(const float* residuals, int C, const uint8_t* mask, int D, int H, int W, float half_range, int bins,
                           long long* hist, long long* counts, double* sums, int records_before, void* ws, size_t ws_bytes,
                           void* stream) {
    if (!residuals || !hist || !counts || !sums || !ws) return fail("irs_residual_histogram: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (bins < IRS_RESIDUAL_MIN_BINS || bins > IRS_RESIDUAL_MAX_BINS)
        return fail("irs_residual_histogram: bins = %d, %d..%d", bins, IRS_RESIDUAL_MIN_BINS, IRS_RESIDUAL_MAX_BINS);
    if (!positive_finite(half_range))
        return fail("irs_residual_histogram: half_range = %g, a finite value > 0 needed", (double)half_range);
    ResBins bn;
    bn.bins = bins;
    bn.half_range = half_range;
    bn.inv_w = (float)bins / (2.0f * half_range);  // fp32, as the definition states it
    if (!positive_finite(bn.inv_w))
        return fail("irs_residual_histogram: half_range = %g is too wide or too narrow for float32 bins", (double)half_range);
    if (!local_dims_ok(__func__, D, H, W)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 record count")) return 1;
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_RESIDUAL_WS_BYTES, "IRS_RESIDUAL_WS_BYTES")) return 1;
    launch_residual_histogram(residuals, mask, (int64_t)D * H * W, C, bn, hist, counts, sums, records_before, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_residual_nll_update(const float* residuals, int C, int D, int H, int W, const double* log_weight, const double* inv_std,
                            int K, float* mean, int32_t* count, int records_before, void* stream) {
    if (!residuals || !log_weight || !inv_std || !mean || !count) return fail("irs_residual_nll_update: bad arguments");
    if (!chains_ok(__func__, C)) return 1;
    if (K < 1 || K > IRS_MAX_COMPONENTS) return fail("irs_residual_nll_update: K = %d components, 1..%d", K, IRS_MAX_COMPONENTS);
    ResMixture mix;
    memset(&mix, 0, sizeof(mix));
    mix.K = K;
    for (int k = 0; k < K; ++k) {
        if (!isfinite(log_weight[k])) return fail("irs_residual_nll_update: log_weight[%d] = %g, a finite value needed", k, log_weight[k]);
        if (!(inv_std[k] > 0.0) || !isfinite(inv_std[k]))
            return fail("irs_residual_nll_update: inv_std[%d] = %g, a finite value > 0 needed", k, inv_std[k]);
        mix.log_weight[k] = log_weight[k];
        mix.inv_std[k] = inv_std[k];
    }
    if (!local_dims_ok(__func__, D, H, W)) return 1;
    if (!records_ok(__func__, records_before, C, INT32_MAX, "overflow the int32 sample count")) return 1;
    launch_residual_nll_update(residuals, C, (int64_t)D * H * W, mix, mean, count, records_before, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_residual_nll_finalize(const float* mean, const int32_t* count, const uint8_t* mask, int D, int H, int W,
                              long long* isummary, double* fsummary, void* ws, size_t ws_bytes, void* stream) {
    if (!mean || !count || !isummary || !fsummary || !ws) return fail("irs_residual_nll_finalize: bad arguments");
    if (!local_dims_ok(__func__, D, H, W)) return 1;
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_RESIDUAL_MAP_WS_BYTES, "IRS_RESIDUAL_MAP_WS_BYTES")) return 1;
    launch_residual_nll_finalize(mean, count, (int64_t)D * H * W, mask, isummary, fsummary, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// coarse-to-fine start (multires_kernels.hip)
// ================================================================================================
// `volumes` volumes go between the fine and the coarse grid; `out_planes`: the first extent of the grid that is written (one
// launch row per volume and plane of it)
static bool multires_ok(const char* who, const void* in, const void* out, int64_t volumes, const int fine[3], const int coarse[3],
                        int out_planes) {
    if (!in || !out) return !fail("%s: null pointer", who);
    const int* grids[2] = {fine, coarse};
    const char* names[2] = {"fine", "coarse"};
    for (int g = 0; g < 2; ++g)
        if (grids[g][0] < 2 || grids[g][1] < 2 || grids[g][2] < 2)
            return !fail("%s: %s dims (%d, %d, %d), every one >= 2 needed", who, names[g], grids[g][0], grids[g][1], grids[g][2]);
    for (int a = 0; a < 3; ++a)
        if (coarse[a] > fine[a])
            return !fail("%s: coarse dims (%d, %d, %d) exceed the fine dims (%d, %d, %d) on axis %d", who, coarse[0], coarse[1],
                         coarse[2], fine[0], fine[1], fine[2], a);
    if ((int64_t)fine[0] * fine[1] * fine[2] >= ((int64_t)1 << 30)) return !fail("%s: the fine volume must have fewer than 2^30 voxels", who);
    return volumes * out_planes <= 65535 ||
           !fail("%s: %lld volumes of %d planes are more than the 65535 rows of one launch", who, (long long)volumes, out_planes);
}

int irs_restrict_image(const float* im, int Cim, int D, int H, int W, float* out, int d, int h, int w, void* stream) {
    if (Cim < 1) return fail("irs_restrict_image: Cim = %d volumes, at least 1 needed", Cim);
    const int fine[3] = {D, H, W}, coarse[3] = {d, h, w};
    if (!multires_ok(__func__, im, out, Cim, fine, coarse, d)) return 1;
    launch_restrict_image(im, out, Cim, make_vol(D, H, W), make_vol(d, h, w), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_restrict_mask(const uint8_t* mask, int Cm, int D, int H, int W, uint8_t* out, int d, int h, int w, void* stream) {
    if (Cm < 1) return fail("irs_restrict_mask: Cm = %d volumes, at least 1 needed", Cm);
    const int fine[3] = {D, H, W}, coarse[3] = {d, h, w};
    if (!multires_ok(__func__, mask, out, Cm, fine, coarse, d)) return 1;
    launch_restrict_mask(mask, out, Cm, make_vol(D, H, W), make_vol(d, h, w), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_prolong_field(const float* x, int C, int ch, int d, int h, int w, float* out, int D, int H, int W, void* stream) {
    if (C < 1 || ch < 1) return fail("irs_prolong_field: C = %d chains of ch = %d channels, at least 1 each needed", C, ch);
    const int fine[3] = {D, H, W}, coarse[3] = {d, h, w};
    if (!multires_ok(__func__, x, out, (int64_t)C * ch, fine, coarse, D)) return 1;
    launch_prolong_field(x, out, C * ch, make_vol(d, h, w), make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// adaptive pSGLD preconditioner (precond_kernels.hip)
// ================================================================================================
static bool precond_grid_ok(const char* who, int D, int H, int W) {
    if (D < 1 || H < 1 || W < 1) return !fail("%s: dims (%d, %d, %d), every one >= 1 needed", who, D, H, W);
    if ((int64_t)D * H * W >= ((int64_t)1 << 30)) return !fail("%s: the volume must have fewer than 2^30 voxels", who);
    return ((H + 7) / 8 <= 65535 && 3 * (((int64_t)D + 3) / 4) <= 65535) ||
           !fail("%s: dims (%d, %d, %d) exceed the launch grid", who, D, H, W);
}

// [a, a + na) and [b, b + nb) floats share an element
static bool floats_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    return (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
}

int irs_precond_workspace(int D, int H, int W, int smooth, size_t* bytes) {
    if (!bytes) return fail("irs_precond_workspace: null pointer");
    if (!precond_grid_ok(__func__, D, H, W)) return 1;
    if (smooth < 0 || smooth > IRS_PRECOND_MAX_SMOOTH)
        return fail("irs_precond_workspace: smooth = %d, 0..%d", smooth, IRS_PRECOND_MAX_SMOOTH);
    *bytes = precond_workspace_bytes(make_vol(D, H, W), smooth);
    return 0;
}

int irs_precond_accumulate(const float* grad_v, const float* sigma, int C, int D, int H, int W, float beta, float* V,
                           long long* nonfinite, void* stream) {
    if (!grad_v || !V || !nonfinite) return fail("irs_precond_accumulate: null pointer");
    if (!chains_ok(__func__, C)) return 1;
    if (!precond_grid_ok(__func__, D, H, W)) return 1;
    if (!(beta >= 0.0f && beta < 1.0f)) return fail("irs_precond_accumulate: beta = %g, a value in [0, 1) needed", (double)beta);
    const int64_t N = (int64_t)3 * D * H * W;
    if (floats_overlap(V, N, grad_v, C * N)) return fail("irs_precond_accumulate: V overlaps grad_v");
    if (sigma && floats_overlap(V, N, sigma, C * N)) return fail("irs_precond_accumulate: V overlaps sigma");
    launch_precond_accumulate(grad_v, sigma, C, N, beta, V, nonfinite, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_precond_sigma(const float* V, int C, int D, int H, int W, double bias, int smooth, double damping, float sigma_min,
                      float sigma_max, const long long* nonfinite, float* sigma, double* summary, void* ws, size_t ws_bytes,
                      void* stream) {
    if (!V || !sigma || !summary || !ws) return fail("irs_precond_sigma: null pointer");
    if (!chains_ok(__func__, C)) return 1;
    if (!precond_grid_ok(__func__, D, H, W)) return 1;
    if (!(bias >= 1.0) || !isfinite((float)bias))
        return fail("irs_precond_sigma: bias = %g, a finite value >= 1 needed (1 / (1 - beta^t))", bias);
    if (smooth < 0 || smooth > IRS_PRECOND_MAX_SMOOTH) return fail("irs_precond_sigma: smooth = %d, 0..%d", smooth, IRS_PRECOND_MAX_SMOOTH);
    if (!(damping > 0.0) || !isfinite(damping)) return fail("irs_precond_sigma: damping = %g, a finite value > 0 needed", damping);
    if (!(sigma_min > 0.0f && sigma_min <= 1.0f && sigma_max >= 1.0f && isfinite(sigma_max)))
        return fail("irs_precond_sigma: sigma_min = %g, sigma_max = %g, 0 < sigma_min <= 1 <= sigma_max < inf needed", (double)sigma_min,
                    (double)sigma_max);
    const Vol vol = make_vol(D, H, W);
    if (!workspace_ok(__func__, ws_bytes, precond_workspace_bytes(vol, smooth), "irs_precond_workspace")) return 1;
    if (floats_overlap(sigma, (int64_t)C * 3 * vol.V, V, 3 * vol.V)) return fail("irs_precond_sigma: sigma overlaps V");
    launch_precond_sigma(V, C, vol, (float)bias, smooth, damping, sigma_min, sigma_max, nonfinite, sigma, summary, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// posterior principal modes (modes_kernels.hip)
// ================================================================================================
static bool modes_grid_ok(const char* who, int D, int H, int W) {
    if (D < 1 || H < 1 || W < 1) return !fail("%s: dims (%d, %d, %d), every one >= 1 needed", who, D, H, W);
    return (int64_t)D * H * W < ((int64_t)1 << 30) || !fail("%s: the volume must have fewer than 2^30 voxels", who);
}

int irs_modes_gram_workspace(int D, int H, int W, int n_new, size_t* bytes) {
    if (!bytes) return fail("irs_modes_gram_workspace: null pointer");
    if (!modes_grid_ok(__func__, D, H, W)) return 1;
    if (n_new < 1 || n_new > IRS_MAX_CHAINS) return fail("irs_modes_gram_workspace: n_new = %d records, 1..%d", n_new, IRS_MAX_CHAINS);
    *bytes = modes_gram_workspace_bytes((int64_t)D * H * W, n_new);
    return 0;
}

int irs_modes_gram_rows(const float* store, int cap, int n_before, int n_new, int D, int H, int W, const uint8_t* mask, double* gram,
                        void* ws, size_t ws_bytes, void* stream) {
    if (!store || !gram || !ws) return fail("irs_modes_gram_rows: null pointer");
    if (cap < 1 || cap > IRS_MODES_MAX_RECORDS) return fail("irs_modes_gram_rows: cap = %d records, 1..%d", cap, IRS_MODES_MAX_RECORDS);
    if (n_new < 1 || n_new > IRS_MAX_CHAINS) return fail("irs_modes_gram_rows: n_new = %d records, 1..%d", n_new, IRS_MAX_CHAINS);
    if (!records_ok(__func__, n_before, n_new, cap, "exceed the store's cap")) return 1;
    if (!modes_grid_ok(__func__, D, H, W)) return 1;
    const int64_t V = (int64_t)D * H * W;
    if (!workspace_ok(__func__, ws_bytes, modes_gram_workspace_bytes(V, n_new), "irs_modes_gram_workspace")) return 1;
    launch_modes_gram_rows(store, cap, n_before, n_new, V, mask, gram, ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_modes_project(const float* store, int n, int D, int H, int W, const double* coeff, int M, const double* scale, float* mean,
                      float* modes, float* explained, void* stream) {
    if (!store || !coeff || !scale || !mean || !modes || !explained) return fail("irs_modes_project: null pointer");
    if (n < 1 || n > IRS_MODES_MAX_RECORDS) return fail("irs_modes_project: n = %d records, 1..%d", n, IRS_MODES_MAX_RECORDS);
    if (M < 1 || M > IRS_MODES_MAX) return fail("irs_modes_project: M = %d modes, 1..%d", M, IRS_MODES_MAX);
    if (!modes_grid_ok(__func__, D, H, W)) return 1;
    for (int a = 0; a < 3; ++a)
        if (!(scale[a] > 0.0) || !isfinite(scale[a]))
            return fail("irs_modes_project: scale[%d] = %g, a finite value > 0 needed", a, scale[a]);
    launch_modes_project(store, n, (int64_t)D * H * W, coeff, M, scale, mean, modes, explained, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// foreground masks (mask_kernels.hip)
// ================================================================================================
int irs_intensity_histogram(const float* im, int C, const uint8_t* mask, int Cm, int D, int H, int W, float lo, float hi, int bins,
                            long long* hist, void* stream) {
    if (!im || !hist) return fail("irs_intensity_histogram: null pointer");
    if (!mask_volumes_ok(__func__, C, D, H, W)) return 1;
    if (mask && !broadcast_ok(Cm, C)) return fail("irs_intensity_histogram: mask of %d volumes, 1 or %d needed", Cm, C);
    if (bins < IRS_MASK_MIN_BINS || bins > IRS_MASK_MAX_BINS)
        return fail("irs_intensity_histogram: bins = %d, %d..%d", bins, IRS_MASK_MIN_BINS, IRS_MASK_MAX_BINS);
    if (!isfinite(lo) || !isfinite(hi) || !(hi > lo))
        return fail("irs_intensity_histogram: range [%g, %g], finite bounds with hi > lo needed", (double)lo, (double)hi);
    const float width = hi - lo;  // fp32, as the definition states it
    const float inv_w = (float)bins / width;
    if (!positive_finite(inv_w))
        return fail("irs_intensity_histogram: range [%g, %g] is too wide or too narrow for float32 bins", (double)lo, (double)hi);
    const int64_t V = (int64_t)D * H * W;
    launch_intensity_histogram(im, mask, mask && Cm == C && C > 1 ? V : 0, V, C, lo, inv_w, bins, hist, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_mask_threshold(const float* im, int C, int D, int H, int W, float threshold, uint8_t* out, void* stream) {
    if (!im || !out) return fail("irs_mask_threshold: null pointer");
    if (!mask_volumes_ok(__func__, C, D, H, W)) return 1;
    if (isnan(threshold)) return fail("irs_mask_threshold: the threshold is NaN");
    launch_mask_threshold(im, threshold, out, C, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

static bool connectivity_ok(const char* who, int connectivity) {
    return connectivity == 6 || connectivity == 18 || connectivity == 26 || !fail("%s: connectivity = %d, 6, 18 or 26", who, connectivity);
}

// the workspace of a mask call: given, 16-byte aligned and of `need` bytes (`hint`: the query that tells them)
static bool mask_workspace_ok(const char* who, const void* ws, size_t have, size_t need, const char* hint) {
    if (!ws) return !fail("%s: null workspace", who);
    if ((uintptr_t)ws & 15) return !fail("%s: the workspace must be 16-byte aligned", who);
    return workspace_ok(who, have, need, hint);
}

int irs_connected_components_workspace(int C, int D, int H, int W, size_t* bytes) {
    if (!bytes) return fail("irs_connected_components_workspace: bad arguments");
    if (!mask_volumes_ok(__func__, C, D, H, W)) return 1;
    *bytes = connected_components_bytes(C, (int64_t)D * H * W);
    return 0;
}

int irs_connected_components(const uint8_t* mask, int C, int D, int H, int W, int connectivity, int32_t* labels, int32_t* counts,
                             void* ws, size_t ws_bytes, void* stream) {
    if (!mask || !labels || !counts) return fail("irs_connected_components: null pointer");
    if (!mask_volumes_ok(__func__, C, D, H, W) || !connectivity_ok(__func__, connectivity)) return 1;
    if (!mask_workspace_ok(__func__, ws, ws_bytes, connected_components_bytes(C, (int64_t)D * H * W), "irs_connected_components_workspace"))
        return 1;
    launch_connected_components(mask, false, connectivity, labels, counts, C, make_vol(D, H, W), ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_mask_select_workspace(int C, int D, int H, int W, size_t* bytes) {
    if (!bytes) return fail("irs_mask_select_workspace: bad arguments");
    if (!mask_volumes_ok(__func__, C, D, H, W)) return 1;
    *bytes = mask_select_bytes(C, (int64_t)D * H * W);
    return 0;
}

int irs_mask_keep_largest(const uint8_t* mask, int C, int D, int H, int W, int connectivity, int keep, uint8_t* out, void* ws,
                          size_t ws_bytes, void* stream) {
    if (!mask || !out) return fail("irs_mask_keep_largest: null pointer");
    if (!mask_volumes_ok(__func__, C, D, H, W) || !connectivity_ok(__func__, connectivity)) return 1;
    if (keep < 1 || keep > IRS_MASK_MAX_KEEP) return fail("irs_mask_keep_largest: keep = %d, 1..%d", keep, IRS_MASK_MAX_KEEP);
    if (!mask_workspace_ok(__func__, ws, ws_bytes, mask_select_bytes(C, (int64_t)D * H * W), "irs_mask_select_workspace")) return 1;
    launch_mask_keep_largest(mask, connectivity, keep, out, C, make_vol(D, H, W), ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_mask_fill_holes(const uint8_t* mask, int C, int D, int H, int W, uint8_t* out, void* ws, size_t ws_bytes, void* stream) {
    if (!mask || !out) return fail("irs_mask_fill_holes: null pointer");
    if (!mask_volumes_ok(__func__, C, D, H, W)) return 1;
    if (!mask_workspace_ok(__func__, ws, ws_bytes, mask_select_bytes(C, (int64_t)D * H * W), "irs_mask_select_workspace")) return 1;
    launch_mask_fill_holes(mask, out, C, make_vol(D, H, W), ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_mask_morphology_workspace(int C, int D, int H, int W, size_t* bytes) {
    if (!bytes) return fail("irs_mask_morphology_workspace: bad arguments");
    if (!mask_volumes_ok(__func__, C, D, H, W)) return 1;
    *bytes = mask_morphology_bytes(C, (int64_t)D * H * W);
    return 0;
}

int irs_mask_dilate(const uint8_t* mask, int C, int D, int H, int W, int r2, int erode, uint8_t* out, void* ws, size_t ws_bytes,
                    void* stream) {
    if (!mask || !out) return fail("irs_mask_dilate: null pointer");
    if (!mask_volumes_ok(__func__, C, D, H, W)) return 1;
    if (r2 < 0 || r2 > IRS_MASK_MAX_RADIUS * IRS_MASK_MAX_RADIUS)
        return fail("irs_mask_dilate: r2 = %d, 0..%d (a radius of at most %d voxels)", r2, IRS_MASK_MAX_RADIUS * IRS_MASK_MAX_RADIUS,
                    IRS_MASK_MAX_RADIUS);
    if (!mask_workspace_ok(__func__, ws, ws_bytes, mask_morphology_bytes(C, (int64_t)D * H * W), "irs_mask_morphology_workspace")) return 1;
    launch_mask_dilate(mask, r2, erode != 0, out, C, make_vol(D, H, W), ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// affine pre-alignment (affine_kernels.hip)
// ================================================================================================
// the volume and the map of an affine call -> `map`; `rows`: launch rows (chains x planes) of the pointwise kernels, 0: none
static bool affine_ok(const char* who, int D, int H, int W, const double* lin, const double* shift, int64_t rows, AffineMap& map) {
    if (!lin || !shift) return !fail("%s: null pointer", who);
    if (D < 2 || H < 2 || W < 2) return !fail("%s: dims (%d, %d, %d), every one >= 2 needed", who, D, H, W);
    if ((int64_t)D * H * W >= ((int64_t)1 << 30)) return !fail("%s: the volume must have fewer than 2^30 voxels", who);
    if (rows > 65535) return !fail("%s: %lld planes are more than the 65535 rows of one launch", who, (long long)rows);
    for (int i = 0; i < 9; ++i) {
        if (!isfinite(lin[i])) return !fail("%s: lin[%d] = %g is not finite", who, i, lin[i]);
        map.lin[i] = lin[i];
    }
    for (int i = 0; i < 3; ++i) {
        if (!isfinite(shift[i])) return !fail("%s: shift[%d] = %g is not finite", who, i, shift[i]);
        map.shift[i] = shift[i];
    }
    return true;
}

int irs_affine_normal_equations(const float* fixed, const float* moving, const uint8_t* mask, int D, int H, int W, const double* lin,
                                const double* shift, double* sums, void* ws, size_t ws_bytes, void* stream) {
    if (!fixed || !moving || !sums || !ws) return fail("irs_affine_normal_equations: null pointer");
    AffineMap map;
    if (!affine_ok(__func__, D, H, W, lin, shift, 0, map)) return 1;
    if (!workspace_ok(__func__, ws_bytes, (size_t)IRS_AFFINE_WS_BYTES, "IRS_AFFINE_WS_BYTES")) return 1;
    if ((uintptr_t)ws & 7) return fail("irs_affine_normal_equations: the workspace must be 8-byte aligned");
    launch_affine_normal_equations(fixed, moving, mask, make_vol(D, H, W), map, sums, (double*)ws, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_affine_transformation(const double* lin, const double* shift, float* out, int D, int H, int W, void* stream) {
    if (!out) return fail("irs_affine_transformation: null pointer");
    AffineMap map;
    if (!affine_ok(__func__, D, H, W, lin, shift, D, map)) return 1;
    launch_affine_transformation(map, out, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_affine_compose(const float* transformation, const double* lin, const double* shift, float* total_transformation,
                       float* total_displacement, int C, int D, int H, int W, void* stream) {
    if (!transformation) return fail("irs_affine_compose: null pointer");
    if (!total_transformation && !total_displacement)
        return fail("irs_affine_compose: total_transformation and total_displacement are both NULL, one is needed");
    if (!chains_ok(__func__, C)) return 1;
    AffineMap map;
    if (!affine_ok(__func__, D, H, W, lin, shift, (int64_t)C * D, map)) return 1;
    launch_affine_compose(transformation, map, total_transformation, total_displacement, C, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

// ================================================================================================
// cubic B-spline output resampling (bspline_kernels.hip)
// ================================================================================================
int irs_bspline_prefilter(const float* im, float* coeff, int Cim, int D, int H, int W, void* stream) {
    if (!im || !coeff) return fail("irs_bspline_prefilter: null pointer");
    if (!chain_count_ok(Cim)) return fail("irs_bspline_prefilter: Cim = %d volumes, 1..%d", Cim, IRS_MAX_CHAINS);
    if (!bspline_volume_ok(__func__, Cim, D, H, W)) return 1;
    launch_bspline_prefilter(im, coeff, Cim, make_vol(D, H, W), (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

int irs_bspline_warp(const float* coeff, int Cim, const float* transformation, float* out, int C, int D, int H, int W, void* stream) {
    if (!coeff || !transformation || !out) return fail("irs_bspline_warp: null pointer");
    if (!chains_ok(__func__, C)) return 1;
    if (!broadcast_ok(Cim, C)) return fail("irs_bspline_warp: coefficients of %d chains, 1 or %d needed", Cim, C);
    if (!bspline_volume_ok(__func__, C, D, H, W)) return 1;
    const Vol vol = make_vol(D, H, W);
    launch_bspline_warp(coeff, Cim == 1 ? 0 : vol.V, transformation, out, C, vol, (hipStream_t)stream);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
