/*
 * irsgmcmc.h -- C ABI of the MI355X-native SG-MCMC registration inner loop.
 *
 * Drop-in boundary for ONE path of dgrzech/ir-sgmcmc: `Trainer._SGLD_transition`
 * (reference trainer/trainer.py:291-356) and the operators it is built from.  The reference has no
 * FFI of its own -- its extension point is name-based construction of Python classes from JSON
 * (parse_config.py:251-266) -- so every entry point below cites the reference call site it replaces.
 * Python binds this header with ctypes (ir_sgmcmc_amd/_lib.py); see INTEGRATION.md.
 *
 * Conventions
 *  - every `float*` / `uint8_t*` argument is a CALLER-OWNED DEVICE pointer (e.g. torch allocation);
 *    fields are planar fp32 (C, 3, D, H, W), images (C, 1, D, H, W), channel 0 = x = last axis
 *    (utils/util.py:263-278); masks are 1 byte per voxel (torch.bool).
 *  - `stream` is a hipStream_t passed as void*; all work is asynchronous on it, nothing synchronises
 *    except the functions documented as "blocking".
 *  - every function returns 0 on success, non-zero on error (irs_last_error() gives the message);
 *    nothing aborts or throws across the boundary; no internal threads.
 *  - a context is not thread-safe; distinct contexts / streams are independent.
 */
#ifndef IRSGMCMC_H
#define IRSGMCMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: these are its only exports */

#define IRS_MAX_COMPONENTS 8
#define IRS_MAX_CHAINS 8
#define IRS_MAX_HALF_WIDTH 4 /* Sobolev / LCC half widths up to 4 */
#define IRS_MAX_LABELS 64    /* labels of one surface-distance call */
#define IRS_HAUSDORFF_MAX_PERCENTILES 4 /* percentiles of one irs_label_hausdorff_distance call */

/* data term (irs_config.data_loss).  The value 2 is reserved: irs_create refuses it. */
enum { IRS_DATA_GMM_LCC = 0, IRS_DATA_SSD = 1, IRS_DATA_LNCC = 3, IRS_DATA_MI = 4, IRS_DATA_NGF = 5 };
enum { IRS_REG_L2 = 0, IRS_REG_LOGNORMAL = 1, IRS_REG_STUDENT = 2, IRS_REG_LOGNORMAL_L2 = 3 };
/* differential operator of the regulariser energy y (irs_config.diff_op): the reference's GradientOperator, or the same
 * operator applied twice (HessianOperator, the bending energy) */
#define IRS_DIFF_GRADIENT 0
#define IRS_DIFF_HESSIAN 1

/* ------------------------------------------------------------------------------------------------
 * stateless operators (unit-parity surface; the Python modules SVF_3D, RegistrationModule, GMM.map,
 * GradientOperator ... call these)
 * ---------------------------------------------------------------------------------------------- */

/* SGLD.forward + SobolevGrad.forward: out = S * (v + sqrt(2 tau) sigma eps)
 * (utils/functions.py:76-84,98-109; utils/util.py:48-58,394-404).
 * v, out, tmp: (C,3,D,H,W).  sigma: NULL (=1) or (C,3,D,H,W).  eps: standard-normal tensor, or NULL ->
 * in-kernel Philox4x32-10 keyed by (seed, iteration), one call per voxel pair (z even, z + 1): six 21-bit words ->
 * three Box-Muller pairs.  kernel: 2s+1 host floats; s == 0 -> no smoothing.
 * tau < 0 -> no noise.  `tmp` may not alias v or out; out may not alias v. */
int irs_perturb_smooth(const float* v, const float* sigma, const float* eps, float tau, const float* kernel, int s,
                       int C, int D, int H, int W, float* tmp, float* out, uint64_t seed, uint64_t iteration,
                       void* stream);

/* One SGHMC step (Chen, Fox & Guestrin 2014, eq. 15 with beta_hat = 0) on (v, momentum) in place, outside a transition.  Per
 * element, float32, every operation rounded once and nothing contracted into an FMA:
 *   t  = fsub(fmul(oma, m), fmul(lr, grad))                    oma = (float)(1 - (double)friction)
 *   m' = T > 0 ? fadd(t, fmul(fmul(amp, sigma), n)) : t        amp = (float)sqrt(2 friction lr T), in double
 *   v' = fadd(v, m')
 * v, momentum, grad: (C,3,D,H,W); grad is what irs_io.grad_v holds (sigma^2 already applied).  sigma: NULL (= 1) or (C,3,D,H,W).
 * n: eps where it is given, else the in-kernel Philox4x32-10 draw of irs_perturb_smooth -- one call per voxel pair (z even, z + 1),
 * the same index and the same assignment of the six normals -- with the stream word 0x484D in place of 0x5347: never a draw the
 * forward perturbation has used.  friction in (0, 1] (1: Langevin dynamics whose noise stays in v), temperature >= 0 (0: no noise
 * is drawn, eps is not read).  Extents >= 1, C in 1..IRS_MAX_CHAINS. */
int irs_sghmc_update(float* v, float* momentum, const float* grad, const float* sigma, const float* eps, int C, int D, int H, int W,
                     float lr, float friction, float temperature, uint64_t seed, uint64_t iteration, void* stream);

/* SVF_3D.forward (utils/transformation.py:63-76): scaling and squaring.
 * v: (C,3,D,H,W) voxel units.  steps: (no_steps, C,3,D,H,W) workspace receiving d_1..d_no_steps in
 * normalised units (kept for the backward).  transformation / displacement: outputs, either may be NULL. */
int irs_svf_exp_fwd(const float* v, float* steps, float* transformation, float* displacement, int no_steps, int C,
                    int D, int H, int W, void* stream);

/* adjoint of the above w.r.t. v (what autograd does through the 12 grid_sample calls).
 * g_last: gradient w.r.t. d_no_steps (normalised units), (C,3,D,H,W).  g_v: output, gradient w.r.t. v.
 * scratch: 2 x (C,3,D,H,W).  Owner-computes gather for max|d_k| < 2 voxels, fixed-point LDS accumulation above: no float
 * atomics, bitwise reproducible. */
int irs_svf_exp_bwd(const float* v, const float* steps, const float* g_last, float* scratch, float* g_v, int no_steps,
                    int C, int D, int H, int W, void* stream);

/* Cubic_B_spline_FFD_3D.forward (utils/transformation.py:126-153) and its adjoint.
 * v_cp: (C,3,G0,G1,G2), G = ceil((N-1)/cps)+3; dense: (C,3,D,H,W); c0, c1, c2: control-point spacing of D, H, W, 1..8.
 * tmp: scratch of irs_ffd_scratch_floats(C, D, H, W, c0, c1, c2) floats, the same for both directions: the two intermediates
 * (C,3,D,G1,G2) and (C,3,D,H,G2).  With cps = 1, or a volume of a few voxels, that is more than 2 x (C,3,D,H,W).
 * irs_ffd_scratch_floats returns 0 for arguments that irs_ffd_up / irs_ffd_adjoint refuse. */
size_t irs_ffd_scratch_floats(int C, int D, int H, int W, int c0, int c1, int c2);
int irs_ffd_up(const float* v_cp, float* dense, float* tmp, int C, int D, int H, int W, int c0, int c1, int c2,
               void* stream);
int irs_ffd_adjoint(const float* g_dense, float* g_cp, float* tmp, int C, int D, int H, int W, int c0, int c1, int c2,
                    void* stream);

/* RegistrationModule.forward, float path (utils/registration.py:29-30) with the optional uniform grid
 * jitter of utils/util.py:44-53 folded in.  im: (Cim,1,D,H,W) with Cim in {1, C} (1 = shared by all chains).
 * d_last: d_no_steps in normalised units (C,3,D,H,W).  unif: U[0,1) tensor (C,3,D,H,W), or NULL -> Philox when
 * alpha > 0.  alpha <= 0 -> no jitter. */
int irs_warp_fwd(const float* im, int Cim, const float* d_last, const float* unif, float alpha, float* warped, int C,
                 int D, int H, int W, uint64_t seed, uint64_t iteration, void* stream);
/* grid-gradient of the warp: g_d = dL/d(d_last) given g_warped (C,1,D,H,W). */
int irs_warp_bwd(const float* im, int Cim, const float* d_last, const float* unif, float alpha, const float* g_warped,
                 float* g_d, int C, int D, int H, int W, uint64_t seed, uint64_t iteration, void* stream);
/* same warp applied to an arbitrary transformation tensor in [-1,1] (the public RegistrationModule call) */
int irs_warp_transformation(const float* im, int Cim, const float* transformation, float* warped, int C, int D, int H,
                            int W, void* stream);
/* nearest-neighbour path for masks (uint8) and label maps (int16) (utils/registration.py:20-27) */
int irs_warp_nearest_u8(const uint8_t* seg, int Cim, const float* transformation, uint8_t* out, int C, int D, int H,
                        int W, void* stream);
int irs_warp_nearest_i16(const int16_t* seg, int Cim, const float* transformation, int16_t* out, int C, int D, int H,
                         int W, void* stream);

/* LCC normalisation (I - u) / sqrt(var + 1e-10) of model/loss.py:103-109; sigma_out may be NULL. */
int irs_lcc_normalise(const float* im, float* out, float* sigma_out, int s, int C, int D, int H, int W, void* stream);
/* GMM.map (model/loss.py:102-111) with the fixed side pre-normalised: z = fhat - LCC(warped).
 * fhat: (Cf,1,D,H,W), Cf in {1,C}.  sigma_m: output, local std of the warped image (kept for the adjoint). */
int irs_lcc_map_fwd(const float* fhat, int Cf, const float* warped, float* z, float* sigma_m, int s, int C, int D,
                    int H, int W, void* stream);
/* adjoint of GMM.map w.r.t. the warped image given g_z. */
int irs_lcc_map_bwd(const float* fhat, int Cf, const float* z, const float* sigma_m, const float* g_z, float* g_warped,
                    int s, int C, int D, int H, int W, void* stream);

/* The LNCC data term (absent in the reference): VoxelMorph's squared local normalised cross-correlation over the (2 radius + 1)^3
 * box window with clamped indices (replicate padding), all of it float32.  With n = (2 radius + 1)^3 and the window sums S_f, S_m,
 * S_ff, S_mm, S_fm of the fixed image F and the moving image M at a voxel,
 *   A = S_fm - S_f S_m / n,  Bf = S_ff - S_f^2 / n,  Bm = S_mm - S_m^2 / n,  den = Bf Bm + eps,  d = 1 - A^2 / den
 * (no special case: a flat window gives d = 1 and gradient 0), and the coefficient maps of the gradient of sum u d,
 *   p = 2 u A / den,  q = 2 u A^2 Bf / den^2,  t = (q S_m - p S_f) / n.
 * fixed: (Cf,1,D,H,W), Cf in {1, C}; moving: (C,1,D,H,W); upstream u: (Cu,1,D,H,W), Cu in {1, C}, or NULL for 1 (Cu ignored);
 * radius 1 .. IRS_MAX_HALF_WIDTH with every dim >= 2 radius + 1; eps finite and > 0.  Outputs, each may be NULL: d (C,1,D,H,W);
 * coef (C,3,D,H,W) = p, q, t; sums: C doubles on the device, sums[c] = sum u d of chain c, which needs partials: scratch of
 * irs_reduce_scratch_doubles() doubles.  No atomics: two calls give the same bits, and chain c of a batch is the single-chain call. */
int irs_lncc_fwd(const float* fixed, int Cf, const float* moving, const float* upstream, int Cu, int radius, float eps,
                 float* d, float* coef, double* sums, double* partials, int C, int D, int H, int W, void* stream);
/* g_moving = d(sum u d)/d(moving) = M box^T(q) - F box^T(p) - box^T(t) from the coefficient maps of irs_lncc_fwd, box^T the adjoint
 * of the clamped box: the padding that was replicated from a face voxel counts there with its multiplicity, on all six faces.
 * g_moving: (C,1,D,H,W), none of the inputs. */
int irs_lncc_bwd(const float* fixed, int Cf, const float* moving, const float* coef, int radius, float* g_moving, int C, int D,
                 int H, int W, void* stream);

/* The mutual-information data term (absent in the reference): a Mattes-style estimator -- zero-order window on the fixed image, cubic
 * B-spline window on the (warped) moving image -- per chain over the n voxels where the mask is set (or absent) and both
 * intensities are finite.  With B = bins in IRS_MI_MIN_BINS .. IRS_MI_MAX_BINS and finite ranges with hi > lo:
 *   fixed bin   a = min(B - 1, max(0, floor((f - f_lo) * (B / (f_hi - f_lo)))))   in float32, the rule of irs_image_similarity
 *   moving      t_raw = (m - m_lo) * ((B - 3) / (m_hi - m_lo)) + 1,  t = clamp(t_raw, 1, B - 2),  k0 = min(floor(t), B - 3),
 *               u = t - k0   in double, every operation rounded once; the taps k0 - 1 .. k0 + 2 always lie in [0, B - 1]
 *   weights     w  = ((1-u)^3, 3u^3 - 6u^2 + 4, -3u^3 + 3u^2 + 3u + 1, u^3) / 6
 *               w' = (-(1-u)^2 / 2, 1.5u^2 - 2u, -1.5u^2 + u + 0.5, u^2 / 2)
 *   fixed point q_j = round(w_j 2^30) for j = 0, 2, 3 and q_1 = 2^30 - q_0 - q_2 - q_3: every voxel adds exactly 2^30 to the
 *               uint64 histogram H, so sum H = n 2^30 as integers
 *   p_ab = H_ab / (n 2^30), p_a and p_b from the integer row and column sums, T_ab = ln(p_ab / (p_a p_b)) (0 where H_ab = 0),
 *   MI = sum p_ab T_ab, a fixed-order double sum; the data term of a chain is weight * n * (ln B - MI) >= 0, and 0 when n = 0.
 *  - irs_mi_fwd.  fixed (Cf,1,D,H,W) float32, Cf in {1, C}; moving (C,1,D,H,W) float32; mask (Cm,1,D,H,W) uint8, Cm in {1, C}, or
 *    NULL (Cm ignored).  Outputs on the device: hist (C,B,B) uint64, may be NULL; table (C,B,B) float32 = T; stats (C,
 *    IRS_MI_STATS) double: n, n_nonfinite (masked voxels with a non-finite intensity), n_clipped (voxels that take part with f
 *    outside [f_lo, f_hi] or t_raw outside [1, B - 2]), MI, H_f, H_m (the entropies of the marginals), the data term at weight 1.
 *    scratch: IRS_MI_WS_BYTES bytes of device memory, 16-byte aligned.  The histogram is zeroed by a memset on the stream in front
 *    of the accumulate kernel and left in place.
 *  - irs_mi_bwd.  table from irs_mi_fwd with the same images, mask, bins and ranges.  g_moving (C,1,D,H,W) float32 =
 *      -scale[c] * mask * inside * (B - 3) / (m_hi - m_lo) * sum_j w'_j(u) T[a][k0 - 1 + j],  inside: 1 <= t_raw <= B - 2,
 *    the gradient of scale[c] * n * (ln B - MI) (n cancels, and so do the marginal terms: sum_j w'_j = 0); exactly 0 where the voxel
 *    does not take part.  scale: C floats on the device, or NULL for 1.  pmi (C,1,D,H,W) float32, may be NULL: sum_j w_j T[a][k0 -
 *    1 + j] at the voxels that take part, 0 elsewhere; in real arithmetic sum pmi = n MI.  Neither output may be an input.
 * Integer histogram, fixed-order sums: two calls give the same bits, and chain c of a batch is the single-chain call. */
#define IRS_MI_STATS 7
#define IRS_MI_MIN_BINS 8
#define IRS_MI_MAX_BINS 64
#define IRS_MI_MAX_BLOCKS 1024 /* rows of per-block counts in the scratch: the accumulate grid has IRS_MI_MAX_BLOCKS / C blocks per chain at most */
#define IRS_MI_WS_BYTES (IRS_MAX_CHAINS * IRS_MI_MAX_BINS * IRS_MI_MAX_BINS * 8 + IRS_MI_MAX_BLOCKS * 3 * 8)
int irs_mi_fwd(const float* fixed, int Cf, const float* moving, const uint8_t* mask, int Cm, int bins, float f_lo, float f_hi,
               float m_lo, float m_hi, uint64_t* hist, float* table, double* stats, void* scratch, int C, int D, int H, int W,
               void* stream);
int irs_mi_bwd(const float* fixed, int Cf, const float* moving, const uint8_t* mask, int Cm, const float* table, int bins, float f_lo,
               float f_hi, float m_lo, float m_hi, const float* scale, float* g_moving, float* pmi, int C, int D, int H, int W,
               void* stream);

/* The NGF data term (absent in the reference): the normalised gradient field distance of Haber & Modersitzki (2006), which compares
 * only the direction of the two image gradients, up to their sign -- local like LNCC, free of a common contrast like MI.  All of
 * it float32.  grad is the central difference with clamped indices, in voxel units, on each of the three axes,
 *   (grad I)_a(x) = 0.5 * (I[min(x_a + 1, n_a - 1)] - I[max(x_a - 1, 0)])        (the replicate padding of the LCC and LNCC windows).
 * With a = grad F (fixed image), b = grad M (moving image) and the edge parameters eps_f, eps_m > 0, at every voxel
 *   P = a.b        Nf = |a|^2 + eps_f^2        Nm = |b|^2 + eps_m^2
 *   r = P / (Nf Nm)        d = 1 - P r                    ( = 1 - (a.b)^2 / (Nf Nm), in [0, 1] )
 *   s = P / Nm             k = -2 u r
 *   c = k (a - s b)                                       ( = u dd/db, three components in the order z, y, x )
 *   g_M = grad^T c                                        ( = d/dM of sum u d )
 * grad^T is the transpose of the clamped difference; on an axis of length n: interior y: 0.5 (c[y-1] - c[y+1]); low face y = 0:
 * 0.5 (-c[0] - c[1]); high face y = n - 1: 0.5 (c[n-2] + c[n-1]); n = 2: the two face rules and nothing else.  The three axes are
 * added in the order z, y, x.  No special case: a flat neighbourhood has P = 0, d = 1 and c = 0, and every denominator is positive.
 * Every operation is rounded once, in the order written (a.b and |a|^2 added left to right over z, y, x; eps^2 a float32 product;
 * the two divisions correctly rounded; nothing contracts into an FMA): a float32 restatement reproduces d, c and g bit for bit
 * (csrc/ngf_device.h spells the operations out).
 *  - irs_ngf_fwd.  fixed: (Cf,1,D,H,W), Cf in {1, C}; moving: (C,1,D,H,W); upstream u: (Cu,1,D,H,W), Cu in {1, C}, or NULL for 1 (Cu
 *    ignored); eps_f, eps_m finite and > 0.  Outputs, each may be NULL: d (C,1,D,H,W); coef (C,3,D,H,W) = c_z, c_y, c_x; sums: C
 *    doubles on the device, sums[c] = sum u d of chain c in a fixed order, which needs partials: scratch of
 *    irs_reduce_scratch_doubles() doubles.
 *  - irs_ngf_bwd.  g_moving (C,1,D,H,W) = grad^T coef, from the coefficient maps alone; g_moving must not be coef.
 * No atomics and no state: two calls give the same bits, and chain c of a batch is the single-chain call. */
int irs_ngf_fwd(const float* fixed, int Cf, const float* moving, const float* upstream, int Cu, float eps_f, float eps_m, float* d,
                float* coef, double* sums, double* partials, int C, int D, int H, int W, void* stream);
int irs_ngf_bwd(const float* coef, float* g_moving, int C, int D, int H, int W, void* stream);

/* GradientOperator + energy (utils/diff_op.py:78-96, model/loss.py:158-159): y[c] = sum (fwd diff)^2.
 * y_out: C doubles on the device.  partials: scratch of irs_reduce_scratch_doubles() doubles. */
int irs_reg_energy(const float* v, double* y_out, double* partials, int C, int D, int H, int W, void* stream);
size_t irs_reduce_scratch_doubles(void);
/* Bending energy: GradientOperator applied twice (forward differences, the difference array replicate-padded, both times),
 * y[c] = sum over component, axis pair (a, b), voxel of (d_a d_b v_comp)^2.  Per component f, w(q) = 2 for q = n - 2, else 1:
 *   pure terms   (f[i+2] - 2 f[i+1] + f[i])^2 for i <= n_a - 3 along every axis a, weight 1;
 *   mixed terms  2 w_a(i) w_b(j) (f[i+1,j+1] - f[i,j+1] - f[i+1,j] + f[i,j])^2 for i <= n_a - 2, j <= n_b - 2, every a < b.
 * v: (C,3,D,H,W); y_out: C doubles on the device; partials: scratch of irs_reduce_scratch_doubles() doubles.  Sums in a fixed
 * order (no atomics): two calls give the same bits. */
int irs_bending_energy(const float* v, double* y_out, double* partials, int C, int D, int H, int W, void* stream);
/* out[c] = scale[c] * d y[c] / d v[c] = scale[c] * 2 H^T W H v[c], the exact adjoint of the above (in the interior the 25-tap
 * stencil {centre 84, axis neighbours -24, axis distance two +2, in-plane diagonals +4} per component).
 * scale: C floats on the device, or NULL for 1; out: (C,3,D,H,W), not v. */
int irs_bending_energy_grad(const float* v, const float* scale, float* out, int C, int D, int H, int W, void* stream);
/* GradientOperator.forward: nabla (C,3,D,H,W,3) as in utils/diff_op.py:92-96; transformation != 0 divides by the
 * pixel spacing 2/(N-1). */
int irs_gradient_operator(const float* v, float* nabla, int transformation, int C, int D, int H, int W, void* stream);
/* calc_det_J of GradientOperator(transformation=True) + NaN count of its log (utils/util.py:72-91,209-212).
 * log_det: (C,1,D,H,W) or NULL; nan_count: C int64 on the device (zeroed by the call). */
int irs_log_det_jacobian(const float* transformation, float* log_det, long long* nan_count, int C, int D, int H, int W,
                         void* stream);

/* Average surface distance of label contours, the ASD half of calc_metrics (utils/util.py:152-206: sitk.LabelContour +
 * HausdorffDistanceImageFilter.GetAverageHausdorffDistance per chain and label), with an exact Euclidean distance transform.
 * seg_fixed: (Cf,1,D,H,W) int16, Cf in {1, C}; seg_moving: (C,1,D,H,W) int16; labels: n_labels (<= IRS_MAX_LABELS) HOST ints.
 * Pair p = c * n_labels + l.  Two steps with one read-back in between:
 *  1. irs_label_boxes: boxes (device, n_pairs x 6 int32) = {zmin, ymin, xmin, zmax, ymax, xmax} (inclusive) of the voxels
 *     labelled labels[l] in seg_fixed[c] or seg_moving[c]; zmin > zmax when there are none.  Every dim >= 1 (the distance
 *     calls below need dims of at least 2, the surface posterior takes the boxes of a thinner volume).
 *  2. the caller copies the boxes to the host; irs_surface_distance_workspace sizes the workspace from that copy;
 *     irs_label_surface_distance takes it (HOST pointer, validated) and writes, per pair, counts[2p] = |A|, counts[2p+1] = |B|
 *     (A, B: contours of the label in seg_fixed / seg_moving) and sums[2p] = sum over A of the distance to B, sums[2p+1] = sum
 *     over B of the distance to A, in spacing units (spacing[0] scales W, [1] H, [2] D).  ASD = (sums[2p] / |A| +
 *     sums[2p+1] / |B|) / 2, infinite when |A| or |B| is 0.  counts / sums: device.  Deterministic (no float atomics).
 *     Blocking only for the upload of a small per-pair table into the head of the workspace; the kernels run asynchronously. */
int irs_label_boxes(const int16_t* seg_fixed, int Cf, const int16_t* seg_moving, const int32_t* labels, int n_labels,
                    int32_t* boxes, int C, int D, int H, int W, void* stream);
int irs_surface_distance_workspace(const int32_t* boxes, int n_pairs, int D, int H, int W, size_t* bytes);
int irs_label_surface_distance(const int16_t* seg_fixed, int Cf, const int16_t* seg_moving, const int32_t* labels,
                               int n_labels, const float* spacing, const int32_t* boxes, void* workspace,
                               size_t workspace_bytes, long long* counts, double* sums, int C, int D, int H, int W,
                               void* stream);

/* Hausdorff and percentile surface distances of the same contours with the same distances (absent in the reference, which
 * logs only the average; sitk.HausdorffDistanceImageFilter.GetHausdorffDistance is the maximum).  Per pair p and direction:
 * S_AB = { d(a, B) : a in A }, S_BA likewise.  The directed percentile q in (0, 100] of a set of n distances is its ascending
 * order statistic of 0-based index k = min(max((int64)ceil(q * (double)n / 100.0) - 1, 0), n - 1), evaluated in double in
 * that order (numpy's method='inverted_cdf'): the smallest distance within which at least q % of the contour voxels lie.  The
 * directed maximum is the percentile at q = 100.  Selection is exact, on the float32 squared distances of the transform; the
 * value written is sqrt((double)d2) of the selected float.
 *  - boxes: from irs_label_boxes, copied to the host, as for irs_label_surface_distance (no other read-back: the ranks are
 *    formed on the device from the counts); irs_hausdorff_workspace sizes the workspace for Q percentiles.
 *  - percentiles: HOST, Q in 0..IRS_HAUSDORFF_MAX_PERCENTILES values, each in (0, 100], strictly increasing.
 *  - counts, sums: as irs_label_surface_distance writes them, bit-identical.
 *  - hd (P,2) doubles: hd[2p] = max over A of d(., B), hd[2p+1] = max over B of d(., A); taken as a maximum of the distances,
 *    not by the selection.  hd_pct (Q,P,2) doubles, [(q * P + p) * 2 + direction]; may be NULL when Q == 0.
 *  - every directed value of a pair is +inf when A or B is empty; NaN is never written.  The symmetric distances are the
 *    larger of the two directions.  Deterministic (integer atomics only, no float atomics).  Device outputs; blocking only
 *    for the upload of the per-pair table. */
int irs_hausdorff_workspace(const int32_t* boxes, int n_pairs, int Q, int D, int H, int W, size_t* bytes);
int irs_label_hausdorff_distance(const int16_t* seg_fixed, int Cf, const int16_t* seg_moving, const int32_t* labels,
                                 int n_labels, const float* spacing, const int32_t* boxes, void* workspace,
                                 size_t workspace_bytes, const double* percentiles, int Q, long long* counts, double* sums,
                                 double* hd, double* hd_pct, int C, int D, int H, int W, void* stream);

/* Surface posterior (absent in the reference): where on the boundary of a structure the chain is unsure, and whether the warped
 * structure is too large or too small there.  At every voxel x of the contour of label l in the shared fixed map, chain c of a
 * recorded step gives the sample s_c(x) = sign * (float)sqrt((double)d2): d2 the float32 squared distance of the transform
 * above from x to the nearest contour voxel of l in seg_moving[c]; sign -1 where seg_moving[c](x) == l (the fixed surface lies
 * inside the warped structure), +1 otherwise; s = 0 where d2 == 0.  A chain whose map holds no voxel of l gives no sample.
 * State: mean, m2 (D,H,W) float32 and count (D,H,W) int32, 12 bytes per voxel (a voxel has one fixed label); zero before the
 * first update.  Every dim >= 1, < 2^30 voxels.
 *  - irs_surface_posterior_update: seg_fixed (1,1,D,H,W) int16, seg_moving (C,1,D,H,W) int16, C in 1 .. IRS_MAX_CHAINS; labels:
 *    1 .. IRS_MAX_LABELS distinct HOST ints; spacing as above; boxes: the HOST copy of irs_label_boxes(seg_fixed, Cf = 1, ...);
 *    irs_surface_posterior_workspace sizes the workspace from it (the bytes of irs_hausdorff_workspace with Q = 0).  At every
 *    fixed-contour voxel of a listed label, for the chains with a sample in ascending order:
 *    k = ++count; delta = s - mean; mean = mean + delta / (float)k; m2 = m2 + delta * (s - mean), every operation rounded once
 *    to float32, none contracted.  Other voxels are never touched.  A gather: each thread owns its voxel, no atomics; two calls
 *    on the same inputs are bit-identical.  Blocking only for the upload of the per-pair table.  count must not pass INT32_MAX.
 *  - irs_surface_posterior_finalize: bias, std (D,H,W) float32, written at every voxel: bias = mean, NaN where count == 0;
 *    std = sqrtf(max(m2, 0) / (float)(count - 1)), NaN where count < 2.  mask (D,H,W) uint8 or NULL (the whole volume).
 *    Per label, over the voxels of its fixed contour inside the mask: isummary (n_labels, IRS_SURFACE_SUMMARY_INTS) int64
 *    {contour voxels, voxels with count >= 1, voxels with count >= 2, then per level q < n_levels the voxels with count >= 2
 *    and |bias| <= z[q] * std, compared in double; the columns of the levels not asked for are 0}; fsummary (n_labels,
 *    IRS_SURFACE_SUMMARY_FLOATS) doubles {sum bias, sum |bias|, sum bias^2, max |bias| over the voxels with count >= 1; sum std,
 *    max std over those with count >= 2}, of the stored float32 values; a maximum nothing entered is -inf.  z: n_levels in
 *    0 .. IRS_SURFACE_MAX_LEVELS HOST doubles, finite and > 0: the half-width of a normal band in standard deviations.  ws:
 *    IRS_SURFACE_WS_BYTES of device memory.  Deterministic (fixed-order sums, no float atomics); no host sync. */
#define IRS_SURFACE_MAX_LEVELS 4
#define IRS_SURFACE_SUMMARY_INTS 7
#define IRS_SURFACE_SUMMARY_FLOATS 6
#define IRS_SURFACE_MAX_BLOCKS 512 /* rows of per-block partials per label in the workspace */
#define IRS_SURFACE_WS_BYTES (IRS_MAX_LABELS * IRS_SURFACE_MAX_BLOCKS * (IRS_SURFACE_SUMMARY_INTS + IRS_SURFACE_SUMMARY_FLOATS) * 8)
int irs_surface_posterior_workspace(const int32_t* boxes, int n_pairs, int D, int H, int W, size_t* bytes);
int irs_surface_posterior_update(const int16_t* seg_fixed, const int16_t* seg_moving, const int32_t* labels, int n_labels,
                                 const float* spacing, const int32_t* boxes, void* workspace, size_t workspace_bytes, float* mean,
                                 float* m2, int32_t* count, int C, int D, int H, int W, void* stream);
int irs_surface_posterior_finalize(const int16_t* seg_fixed, const int32_t* labels, int n_labels, const float* mean, const float* m2,
                                   const int32_t* count, const uint8_t* mask, const double* z, int n_levels, float* bias, float* std,
                                   long long* isummary, double* fsummary, void* ws, size_t ws_bytes, int D, int H, int W,
                                   void* stream);

/* Split-R-hat of a vector field over chains (absent in the reference; Gelman et al., BDA3 section 11.4), from online moments.
 * Layouts: x (C,3,D,H,W) fp32; mean / m2 (2,C,3,D,H,W) fp32, the Welford state of each half of each chain's samples.
 *  - irs_chain_moments_update: folds x into half `half` (0 or 1) of every chain; k >= 1 = samples in that half after this one
 *    (k = 1 overwrites whatever the half held).  One launch.
 *  - irs_split_rhat: n >= 2 = samples per half.  rhat (D,H,W): per voxel the largest over the three components of
 *    sqrt(var+ / W), W = mean of M2 / (n - 1) over the 2C sequences, var+ = (n - 1) / n W + (variance of the sequence means);
 *    1 where W = B = 0, +inf where W = 0 < B; never NaN.  mask (D,H,W) uint8 or NULL (whole volume).  summary: 5 doubles
 *    on the device {voxels in the mask, voxels with rhat > thr0, with rhat > thr1, max, sum of rhat}.  ws: device
 *    workspace of irs_split_rhat_workspace bytes.  Deterministic (fixed-order reduction, no float atomics); no host sync. */
int irs_chain_moments_update(const float* x, int C, int D, int H, int W, int half, int k, float* mean, float* m2, void* stream);
int irs_split_rhat_workspace(int C, int D, int H, int W, size_t* bytes);
int irs_split_rhat(const float* mean, const float* m2, int C, int n, const uint8_t* mask, float thr0, float thr1, float* rhat,
                   double* summary, void* ws, size_t ws_bytes, int D, int H, int W, void* stream);

/* Split effective sample size and MCSE of the posterior mean (absent in the reference; BDA3 section 11.5), from the moments
 * above and an online variogram.  Layouts: x (C,3,D,H,W); ring (L,C,3,D,H,W), the last L samples of the current half;
 * vsum (L,3,D,H,W), vsum[t-1] = sum over both halves and all chains of (x_i - x_{i-t})^2; all fp32.  C <= IRS_MAX_CHAINS.
 *  - irs_chain_variogram_update: k >= 1 = the same k as irs_chain_moments_update (position in the current half after x).
 *    For t = 1 .. min(k-1, L): vsum[t-1] += sum over chains of (x - ring[(k-1-t) mod L])^2; then ring[(k-1) mod L] = x.
 *    One launch, no atomics: two identical call sequences are bit-identical.
 *  - irs_split_ess: n >= 4 samples per half, L >= 1 lags in vsum (L' = min(L, n-1) are used).  Per component
 *    var+ = (n-1)/n W + B/n as for R-hat, rho_t = 1 - vsum[t-1] / (2C (n-t)) / (2 var+), tau = 1 + 2 sum_{t<=T} rho_t with
 *    T the first odd T with T + 2 <= L' and rho_{T+1} + rho_{T+2} < 0 (else the largest odd T <= L': truncated),
 *    ESS = mn / tau capped at mn max(1, log10 mn) (m = 2C), MCSE = sqrt(var+ / ESS).  var+ = 0 gives ESS = mn, MCSE = 0;
 *    non-finite moments or sums give ESS = 0, MCSE = +inf; never NaN.  ess (D,H,W): the smallest over the three components,
 *    mcse (D,H,W): the largest.  mask (D,H,W) uint8 or NULL.  summary: 5 doubles on the device {voxels in the mask, voxels
 *    with ESS < threshold, voxels with a truncated component, min ESS, sum of ESS}.  ws: irs_split_ess_workspace bytes.
 *    Deterministic (fixed-order reduction, no float atomics); no host sync. */
int irs_chain_variogram_update(const float* x, int C, int D, int H, int W, int k, int L, float* ring, float* vsum, void* stream);
int irs_split_ess_workspace(int C, int D, int H, int W, size_t* bytes);
int irs_split_ess(const float* mean, const float* m2, const float* vsum, int C, int n, int L, const uint8_t* mask, float threshold,
                  float* ess, float* mcse, double* summary, void* ws, size_t ws_bytes, int D, int H, int W, void* stream);

/* Posterior label maps of the propagated segmentation (absent in the reference): per-voxel counts of K structures over n
 * records (one chain's nearest-neighbour warp of the moving segmentation at one recorded step), whatever n is.  Structure j
 * is label value labels[j] (HOST int32, K in 1 .. IRS_MAX_LABELS, distinct, in the int16 range); every other value of a map,
 * 0 and negative values included, is the extra class "other".  64-bit indexing throughout.
 *  - irs_label_posterior_update: seg (C,1,D,H,W) int16, C in 1 .. IRS_MAX_CHAINS; counts (K,D,H,W) int32, += 1 where a record
 *    carries the structure; volume (K,2) double {mean, M2}: Welford state of the per-record volumes (voxels carrying the
 *    structure), folded with k = records_before + c + 1 for c = 0 .. C-1 (k = 1 overwrites it).  records_before >= 0 and
 *    records_before + C <= INT32_MAX.  One stream pass plus a one-block fold; no atomics whose result depends on order.
 *  - irs_label_posterior_finalize: n >= 1 records; seg_fixed (D,H,W) int16; mask (D,H,W) uint8 or NULL (whole volume).  Per
 *    voxel, c_other = n - sum_j c_j; entropy (D,H,W) float32: -sum p ln p over the K + 1 classes in nats (in double); map_label
 *    (D,H,W) int16: the label value of the class with the largest count, ties to the first of (other, structure 0, ...),
 *    0 for other.  summary (K, 6 + 3*IRS_LABEL_BINS) int64, y = [seg_fixed = labels[j]]: S0 = |y|, S1 = sum c_j,
 *    S2 = sum c_j y, S3 = |MAP = j|, S4 = |MAP = j and y|, S5 = |0 < c_j < n|, then per bin b = min(c_j B / n, B - 1) of the
 *    pairs with c_j > 0 or y: pairs, sum c_j, sum y.  mask_summary: 4 doubles {voxels in the mask, sum of the stored entropy
 *    over them, its max (0 when empty), voxels anywhere with sum_j c_j > n (non-zero: n is wrong)}.
 *    Deterministic (exact integer sums, fixed-order float sums); no host sync.
 *  ws: device workspace of irs_label_posterior_workspace bytes (it covers both calls for the same C, K and volume). */
#define IRS_LABEL_BINS 10
int irs_label_posterior_workspace(int C, int K, int D, int H, int W, size_t* bytes);
int irs_label_posterior_update(const int16_t* seg, int C, int D, int H, int W, const int32_t* labels, int K, int32_t* counts,
                               double* volume, int records_before, void* ws, size_t ws_bytes, void* stream);
int irs_label_posterior_finalize(const int32_t* counts, int K, int D, int H, int W, int n, const int32_t* labels,
                                 const int16_t* seg_fixed, const uint8_t* mask, float* entropy, int16_t* map_label,
                                 long long* summary, double* mask_summary, void* ws, size_t ws_bytes, void* stream);

/* Jacobian posterior maps (absent in the reference, which turns log det J into one fold count per sample at its call site
 * utils/util.py:72-91,209-212): per voxel, over n records (one chain's transformation at one recorded step), the number of
 * folded records and the Welford mean / M2 of log det J over the others, whatever n is.  det J is the one irs_log_det_jacobian
 * computes (the same device function); a record is folded at a voxel when !(det > 0), i.e. det <= 0 or NaN -- the per-sample
 * NaN count of irs_log_det_jacobian leaves out det == 0 exactly, whose log is -inf.
 *  - irs_jacobian_posterior_update: transformation (C,3,D,H,W) float32 in [-1,1] coordinates, C in 1 .. IRS_MAX_CHAINS,
 *    every dim >= 2; folds (D,H,W) int32, mean and m2 (D,H,W) float32, updated in place with the C records in chain order.
 *    records_before >= 0 records were folded in before, records_before + C <= INT32_MAX; records_before = 0 overwrites the
 *    fold count, and a voxel's first valid record (records_before - folds = 0 before it) overwrites its mean / m2.  One
 *    launch, one voxel per thread, no atomics.
 *  - irs_jacobian_posterior_finalize: n >= 1 records, k = n - folds valid ones.  fold_prob (D,H,W) float32 = folds / n
 *    (divided in double); logJ_mean = mean and logJ_std = sqrt(m2 / max(k - 1, 1)), NaN where k < 1.  mask (D,H,W) uint8 or
 *    NULL (whole volume).  isummary: IRS_JACOBIAN_SUMMARY_INTS int64 over the mask {voxels, voxels with folds > 0, voxels with
 *    k < 1, sum of folds}.  fsummary: IRS_JACOBIAN_SUMMARY_FLOATS doubles over the stored float32 maps in the mask {max
 *    fold_prob, min logJ_mean, max logJ_mean, sum of logJ_std, max logJ_std}, the last four over voxels with k >= 1; a
 *    maximum nothing entered is -inf, a minimum +inf.  ws: IRS_JACOBIAN_WS_BYTES of device memory.  Deterministic (exact
 *    integer sums, fixed-order double sums and min / max); no host sync. */
#define IRS_JACOBIAN_SUMMARY_INTS 4
#define IRS_JACOBIAN_SUMMARY_FLOATS 5
#define IRS_JACOBIAN_WS_BYTES (1024 * (IRS_JACOBIAN_SUMMARY_INTS + IRS_JACOBIAN_SUMMARY_FLOATS) * 8)
int irs_jacobian_posterior_update(const float* transformation, int C, int D, int H, int W, int32_t* folds, float* mean, float* m2,
                                  int records_before, void* stream);
int irs_jacobian_posterior_finalize(const int32_t* folds, const float* mean, const float* m2, int D, int H, int W, int n,
                                    const uint8_t* mask, float* fold_prob, float* logJ_mean, float* logJ_std, long long* isummary,
                                    double* fsummary, void* ws, size_t ws_bytes, void* stream);

/* Image posterior (absent in the reference): S volumes that live on the moving image's grid, carried through every recorded
 * transformation; per voxel of the fixed grid and volume, over n records (one chain's transformation at one recorded step), the
 * Welford mean / M2, the minimum and the maximum of the trilinear sample, whatever n is: 16 S bytes per voxel.
 *  - irs_image_posterior_update: volumes (S,1,D,H,W) float32 shared by the chains, S in 1 .. IRS_IMAGE_POSTERIOR_MAX_VOLUMES;
 *    transformation (C,3,D,H,W) float32 in [-1,1] coordinates, C in 1 .. IRS_MAX_CHAINS, every dim >= 2: what
 *    irs_warp_transformation takes, and the sample x is bit for bit the value that call writes (same expressions, border clamp;
 *    a tap read with weight 0 still carries a NaN, 0 * NaN, as it does there).  mean, m2, low, high (S,D,H,W) float32, updated
 *    in place with the C records in chain order: k = records_before + c + 1, d = x - mean, mean += d / (float)k,
 *    m2 += d * (x - mean), low = fminf(low, x), high = fmaxf(high, x).  records_before >= 0 records were folded in before,
 *    records_before + C <= INT32_MAX; records_before = 0 overwrites the state (mean = low = high = x, m2 = 0), which is then
 *    never read.  A non-finite sample leaves the voxel's mean non-finite for good.  One launch: a thread owns one voxel of a
 *    group of volumes, forms the taps and weights of a chain once for all of them and keeps their state in registers; no atomics.
 *  - irs_image_posterior_finalize: ONE volume's four state planes (D,H,W) after n >= 1 records.  std_out = sqrtf(m2 /
 *    max(n - 1, 1)), range_out = high - low; with reference (D,H,W) float32, z_out = (reference - mean) / sqrtf(std^2 +
 *    std_floor^2), std_floor finite and >= 0: the misfit of the posterior-mean image in units of the spread the registration
 *    uncertainty explains.  reference and z_out are both NULL or both given.  A voxel with a non-finite mean gets NaN in every
 *    map.  mask (D,H,W) uint8 or NULL (whole volume).  isummary: IRS_IMAGE_POSTERIOR_SUMMARY_INTS int64 over the mask {voxels,
 *    voxels with a non-finite mean, voxels with |z| > 2, voxels with |z| > 3}.  fsummary: IRS_IMAGE_POSTERIOR_SUMMARY_FLOATS
 *    doubles over the stored float32 maps of the other masked voxels {sum mean, sum std, max std, max range, sum z^2, max |z|};
 *    a NaN z (0 / 0) enters no z column; a maximum nothing entered is -inf; without a reference the z counts are 0 and the two
 *    z columns NaN.  ws: IRS_IMAGE_POSTERIOR_WS_BYTES of device memory.  Deterministic (exact integer sums, fixed-order double
 *    sums and maxima); no host sync. */
#define IRS_IMAGE_POSTERIOR_MAX_VOLUMES 8
#define IRS_IMAGE_POSTERIOR_SUMMARY_INTS 4
#define IRS_IMAGE_POSTERIOR_SUMMARY_FLOATS 6
#define IRS_IMAGE_POSTERIOR_WS_BYTES (1024 * (IRS_IMAGE_POSTERIOR_SUMMARY_INTS + IRS_IMAGE_POSTERIOR_SUMMARY_FLOATS) * 8)
int irs_image_posterior_update(const float* volumes, int S, const float* transformation, int C, int D, int H, int W, float* mean,
                               float* m2, float* low, float* high, int records_before, void* stream);
int irs_image_posterior_finalize(const float* mean, const float* m2, const float* low, const float* high, int D, int H, int W, int n,
                                 const float* reference, float std_floor, const uint8_t* mask, float* std_out, float* range_out,
                                 float* z_out, long long* isummary, double* fsummary, void* ws, size_t ws_bytes, void* stream);

/* Displacement covariance posterior (absent in the reference, whose displacement std is three per-component numbers): per
 * voxel, over n records (one chain's displacement at one recorded step, pooled over chains), the Welford mean and the six
 * co-moments of the displacement, and from them the principal spreads and the major direction of its 3 x 3 sample covariance.
 *  - irs_displacement_covariance_update: displacement (C,3,D,H,W) float32 in normalised coordinates, C in 1 ..
 *    IRS_MAX_CHAINS, every dim >= 2; mean (3,D,H,W) and comoment (6,D,H,W: xx, yy, zz, xy, xz, yz) float32, updated in place
 *    with the C records in chain order: delta_a = x_a - mean_a, mean_a += delta_a / (float)k, comoment_ab += delta_a *
 *    (x_b - mean_b) with the new mean_b.  records_before >= 0 records were folded in before, records_before + C <= INT32_MAX;
 *    records_before = 0 overwrites the state (mean = x, comoment = 0), which is then never read.  Non-finite inputs propagate.
 *    One launch, each thread owns its voxels, no atomics.
 *  - irs_displacement_covariance_finalize: n >= 1 records; scale: 3 host floats, finite and > 0, one per channel.  Per voxel,
 *    in double, S_ab = scale_a scale_b comoment_ab / max(n - 1, 1) is diagonalised by 5 cyclic Jacobi sweeps over the pairs
 *    (0,1), (0,2), (1,2); the eigenvalues are sorted descending and clamped at 0.  std (3,D,H,W) float32: their square roots.
 *    direction (3,D,H,W) float32: the unit eigenvector of the largest one, its stored component of largest magnitude positive
 *    (the lowest channel on a tie), the zero vector where that eigenvalue is 0.  anisotropy (D,H,W) float32: the fractional
 *    anisotropy sqrt(3/2 sum (l_i - mean l)^2 / sum l_i^2), 0 where the denominator is 0.  A voxel whose state holds a
 *    non-finite value gives NaN in all seven planes.  mask (D,H,W) uint8 or NULL (whole volume).  isummary:
 *    IRS_COVARIANCE_SUMMARY_INTS int64 over the mask {voxels, voxels with a non-finite state}.  fsummary:
 *    IRS_COVARIANCE_SUMMARY_FLOATS doubles over the stored float32 maps of the other masked voxels {sum std[0], max std[0],
 *    sum sqrt(std[0]^2 + std[1]^2 + std[2]^2), sum anisotropy, max anisotropy, sum |direction[0]|, sum |direction[1]|,
 *    sum |direction[2]|}; a maximum nothing entered is -inf.  ws: IRS_COVARIANCE_WS_BYTES of device memory.  Deterministic
 *    (exact integer sums, fixed-order double sums and maxima); no host sync. */
#define IRS_COVARIANCE_SUMMARY_INTS 2
#define IRS_COVARIANCE_SUMMARY_FLOATS 8
#define IRS_COVARIANCE_WS_BYTES (1024 * (IRS_COVARIANCE_SUMMARY_INTS + IRS_COVARIANCE_SUMMARY_FLOATS) * 8)
int irs_displacement_covariance_update(const float* displacement, int C, int D, int H, int W, float* mean, float* comoment,
                                       int records_before, void* stream);
int irs_displacement_covariance_finalize(const float* mean, const float* comoment, int D, int H, int W, int n, const float* scale,
                                         const uint8_t* mask, float* std, float* direction, float* anisotropy, long long* isummary,
                                         double* fsummary, void* ws, size_t ws_bytes, void* stream);

/* Posterior comparison (absent in the reference, which writes the VI and the MCMC displacement std and compares nothing): per
 * voxel, the distances between the 3-D Gaussians fitted to two states A and B of irs_displacement_covariance_update.
 *  - irs_posterior_compare: mean_x (3,D,H,W) and comoment_x (6,D,H,W: xx, yy, zz, xy, xz, yz) float32 after n_x >= 2 records,
 *    every dim >= 2; scale: 3 host floats, finite and > 0, one per channel (s); std_floor: f, finite and > 0.  Per voxel, in
 *    double: S_X = diag(s) comoment_X diag(s) / (n_X - 1), Delta = s o (mean_A - mean_B); S_A and S_B are diagonalised by the 5
 *    cyclic Jacobi sweeps of irs_displacement_covariance_finalize, eigenvalues clamped at 0.  Four (D,H,W) float32 planes:
 *    shift = |Delta|_2.  log_std_ratio = 1/2 ln(t_A / t_B), t_X = max(tr S_X, 3 f^2): negative where A is the narrower;
 *    exactly 0 for t_A == t_B and exactly antisymmetric under A <-> B.  bures = sqrt(max(tr S_A + tr S_B - 2 sum_i
 *    sqrt(max(lambda_i(R), 0)), 0)), R = S_B^1/2 S_A S_B^1/2, formed symmetric in B's eigenbasis and diagonalised by the same
 *    sweeps; no floor (the 2-Wasserstein distance of the two Gaussians is sqrt(shift^2 + bures^2)).  jeffreys = 1/2 [tr(S~_B^-1
 *    S~_A) + tr(S~_A^-1 S~_B) - 6 + Delta^T (S~_A^-1 + S~_B^-1) Delta] = KL(A|B) + KL(B|A), S~_X = S_X with every eigenvalue
 *    raised to at least f^2.  A voxel with a non-finite value among its 18 state values gives NaN in all four planes.  mask
 *    (D,H,W) uint8 or NULL (whole volume).  isummary: IRS_COMPARE_SUMMARY_INTS int64 over the mask {voxels, voxels with a
 *    non-finite state, voxels where one of the six eigenvalues was raised to f^2, voxels with log_std_ratio < 0}.  fsummary:
 *    IRS_COMPARE_SUMMARY_FLOATS doubles over the stored float32 planes of the finite masked voxels {sum shift, max shift, sum
 *    log_std_ratio, min log_std_ratio, max log_std_ratio, sum bures, max bures, sum w2, max w2 (w2 = sqrt(shift^2 + bures^2)),
 *    sum jeffreys, max jeffreys, sum tr S_A, sum tr S_B}; a maximum nothing entered is -inf, a minimum +inf.  ws:
 *    IRS_COMPARE_WS_BYTES of device memory.  One launch and one finish launch.  Deterministic (exact integer sums, fixed-order
 *    double sums and extrema); no host sync. */
#define IRS_COMPARE_SUMMARY_INTS 4
#define IRS_COMPARE_SUMMARY_FLOATS 13
#define IRS_COMPARE_WS_BYTES (1024 * (IRS_COMPARE_SUMMARY_INTS + IRS_COMPARE_SUMMARY_FLOATS) * 8)
int irs_posterior_compare(const float* mean_a, const float* comoment_a, int n_a, const float* mean_b, const float* comoment_b, int n_b,
                          int D, int H, int W, const float* scale, double std_floor, const uint8_t* mask, float* shift,
                          float* log_std_ratio, float* bures, float* jeffreys, long long* isummary, double* fsummary, void* ws,
                          size_t ws_bytes, void* stream);

/* Displacement credible intervals (absent in the reference, which keeps moments only): per voxel and channel a histogram of
 * the displacement over the records (one chain's displacement at one recorded step, pooled over chains), and from it the
 * quantiles of given probabilities and the width of the band between the first and the last of them.
 *  - irs_displacement_quantiles_update: displacement (C,3,D,H,W) float32 in normalised coordinates, C in 1 ..
 *    IRS_MAX_CHAINS, every dim >= 2; centre (3,D,H,W) float32; hist (3,bins,D,H,W) uint16, bin-major; bins even in
 *    IRS_QUANTILE_MIN_BINS .. IRS_QUANTILE_MAX_BINS; inv_width: 3 host floats, finite and > 0, one per channel.  Every record
 *    adds one count per voxel and channel a to the bin, in float32,
 *        t = floorf((x_a - centre_a) * inv_width_a);  t = fminf(fmaxf(t, -bins), bins);  bin = min(max((int)t + bins / 2, 0), bins - 1)
 *    so bin b with 0 < b < bins - 1 covers [centre + (b - bins/2) w, centre + (b - bins/2 + 1) w) and bins 0 and bins - 1 are
 *    open-ended; a NaN counts into bin 0.  records_before = 0 writes centre from chain 0 and overwrites hist, which is then
 *    never read.  records_before >= 0 and records_before + C <= IRS_QUANTILE_MAX_RECORDS, so a count never wraps.  Counts
 *    commute: the histogram does not depend on the order of chains or steps.  One launch, each thread owns its voxels, no atomics.
 *  - irs_displacement_quantiles_finalize: n in 1 .. IRS_QUANTILE_MAX_RECORDS records; width, scale: 3 host floats each,
 *    finite and > 0; probs: P host doubles, 2 <= P <= IRS_QUANTILE_MAX_PROBS, strictly increasing in (0,1).  Per voxel,
 *    channel and probability p, with r = p n in double and b the first bin whose cumulative count cum_b >= r:
 *        q = scale_a (centre_a + ((b - bins/2) + (r - cum_{b-1}) / count_b) width_a)
 *    in double, stored as float32, NaN (out of range) where b is 0 or bins - 1.  quantiles (P,3,D,H,W) float32.  ci_width
 *    (D,H,W) float32: sqrt(sum_a (q_last,a - q_first,a)^2) of the stored quantiles, in double; NaN where any quantile of the
 *    voxel is.  mask (D,H,W) uint8 or NULL (whole volume).  isummary: IRS_QUANTILE_SUMMARY_INTS int64 over the mask {voxels,
 *    voxels with an out-of-range quantile, samples in bins 0 and bins - 1 summed over the channels}.  fsummary:
 *    IRS_QUANTILE_SUMMARY_FLOATS doubles over the stored float32 maps of the other masked voxels {sum ci_width, max ci_width,
 *    sum |q_last - q_first| of channel 0, 1, 2}; a maximum nothing entered is -inf.  ws: IRS_QUANTILE_WS_BYTES of device
 *    memory.  Deterministic (exact integer sums, fixed-order double sums and maxima); no host sync. */
#define IRS_QUANTILE_MIN_BINS 4
#define IRS_QUANTILE_MAX_BINS 256 /* bins even */
#define IRS_QUANTILE_MAX_PROBS 8
#define IRS_QUANTILE_MAX_RECORDS 65535
#define IRS_QUANTILE_SUMMARY_INTS 3
#define IRS_QUANTILE_SUMMARY_FLOATS 5
#define IRS_QUANTILE_WS_BYTES (1024 * (IRS_QUANTILE_SUMMARY_INTS + IRS_QUANTILE_SUMMARY_FLOATS) * 8)
int irs_displacement_quantiles_update(const float* displacement, int C, int D, int H, int W, float* centre, uint16_t* hist,
                                      int bins, const float* inv_width, int records_before, void* stream);
int irs_displacement_quantiles_finalize(const float* centre, const uint16_t* hist, int bins, int D, int H, int W, int n,
                                        const float* width, const float* scale, const double* probs, int P, const uint8_t* mask,
                                        float* quantiles, float* ci_width, long long* isummary, double* fsummary, void* ws,
                                        size_t ws_bytes, void* stream);

/* Inverse transformation and inverse-consistency error (absent in the reference, which only evaluates the forward map).  For
 * a stationary velocity field exp(-v) is the inverse of exp(v); how well the squaring steps at fp32 invert is what the error
 * maps say.
 *  - irs_svf_exp_inverse: exp(-v) by scaling and squaring.  v (C,3,D,H,W) float32 in voxel units, every dim >= 2, no_steps in
 *    1 .. 30, as irs_svf_exp_fwd; scratch: 2 x (C,3,D,H,W) float32 workspace (two fields, not no_steps of them: nothing is
 *    kept for a backward).  -v is written into scratch[1]; step 0 reads it and writes scratch[0], later steps ping-pong.
 *    transformation ([-1,1] coordinates) / displacement (voxels): (C,3,D,H,W) outputs, either may be NULL.  The launches are
 *    those of irs_svf_exp_fwd: bit-identical to irs_svf_exp_fwd called on -v.  Deterministic; no host sync.
 *  - irs_inverse_consistency: per chain and voxel x, r = d_a(x) + trilinear(d_b)(t_a(x)).  t_a (C,3,D,H,W) float32: a
 *    transformation in [-1,1] coordinates; d_a, d_b (C,3,D,H,W) float32: displacements in one common linear unit (the
 *    `displacement` outputs are in voxels); C in 1 .. IRS_MAX_CHAINS, every dim >= 2.  The three channels of d_b are sampled
 *    at t_a(x) with the trilinear sampler of the squaring step and the warp (border clamp, align_corners, the same
 *    expressions).  residual (C,3,D,H,W) float32 or NULL: r.  norm (C,1,D,H,W) float32 or NULL: sqrt(sum_c (scale_c r_c)^2),
 *    every product, sum and the root rounded to float32 in that order.  scale: 3 host floats, finite and > 0, one per
 *    channel.  mask: uint8, (mask_chains,1,D,H,W) with mask_chains 1 (shared) or C, or NULL (whole volume; mask_chains is
 *    then ignored).  isummary (C, IRS_ICE_SUMMARY_INTS) int64 per chain over the mask {voxels, voxels with a non-finite
 *    norm}; fsummary (C, IRS_ICE_SUMMARY_FLOATS) doubles over the other masked voxels {sum norm, sum norm^2, max norm}; a
 *    maximum nothing entered is -inf.  ws: IRS_ICE_WS_BYTES of device memory.  Called as (t, d, d_inv) of (phi, phi^-1) it
 *    gives phi^-1 o phi - id on the fixed grid; as (t_inv, d_inv, d) it gives phi o phi^-1 - id on the moving grid.
 *    Deterministic (exact integer sums, fixed-order double sums and maxima: one row of partials per block, one reduce per
 *    chain); no atomics; no host sync.
 *  - irs_inverse_consistency_update: norm (C,1,D,H,W) float32, C in 1 .. IRS_MAX_CHAINS; mean, peak (D,H,W) float32, updated
 *    in place with the C maps in chain order: k = records_before + c + 1, mean += (x - mean) / (float)k (k = 1: mean = x),
 *    peak = fmaxf(peak, x) over the finite x only.  records_before >= 0, records_before + C <= INT32_MAX; records_before = 0
 *    overwrites the state, which is then never read.  Non-finite values propagate into mean; peak is NaN where no value
 *    was ever finite.  One launch, each thread owns its voxels, no atomics; no host sync.
 *  - irs_inverse_consistency_finalize: masked summary of the two maps.  mask (D,H,W) uint8 or NULL (whole volume); threshold:
 *    finite and > 0, in the unit of the maps.  isummary: IRS_ICE_MAP_SUMMARY_INTS int64 over the mask {voxels, voxels with a
 *    non-finite mean, voxels with peak > threshold}; fsummary: IRS_ICE_MAP_SUMMARY_FLOATS doubles {sum mean, max mean} over
 *    the masked voxels with a finite mean and {max peak} over those with a finite peak; a maximum nothing entered is -inf.
 *    ws: IRS_ICE_MAP_WS_BYTES of device memory.  Deterministic (exact integer sums, fixed-order double sums and maxima); no
 *    host sync. */
#define IRS_ICE_SUMMARY_INTS 2
#define IRS_ICE_SUMMARY_FLOATS 3
#define IRS_ICE_WS_BYTES (IRS_MAX_CHAINS * 1024 * (IRS_ICE_SUMMARY_INTS + IRS_ICE_SUMMARY_FLOATS) * 8)
#define IRS_ICE_MAP_SUMMARY_INTS 3
#define IRS_ICE_MAP_SUMMARY_FLOATS 3
#define IRS_ICE_MAP_WS_BYTES (1024 * (IRS_ICE_MAP_SUMMARY_INTS + IRS_ICE_MAP_SUMMARY_FLOATS) * 8)
int irs_svf_exp_inverse(const float* v, float* scratch, float* transformation, float* displacement, int no_steps, int C, int D,
                        int H, int W, void* stream);
int irs_inverse_consistency(const float* t_a, const float* d_a, const float* d_b, const float* scale, const uint8_t* mask,
                            int mask_chains, float* residual, float* norm, long long* isummary, double* fsummary, void* ws,
                            size_t ws_bytes, int C, int D, int H, int W, void* stream);
int irs_inverse_consistency_update(const float* norm, int C, int D, int H, int W, float* mean, float* peak, int records_before,
                                   void* stream);
int irs_inverse_consistency_finalize(const float* mean, const float* peak, int D, int H, int W, const uint8_t* mask,
                                     float threshold, long long* isummary, double* fsummary, void* ws, size_t ws_bytes,
                                     void* stream);

/* Native-resolution outputs (absent in the reference, whose outputs all live on the registration grid): a sampled
 * transformation applied on the image's own voxel grid.  The data set pads the native volume `native` = (n0, n1, n2) by
 * `padding` = (p0, p1, p2) voxels on both sides of each axis (P_a = n_a + 2 p_a) and resizes the padded volume to the
 * registration grid `dims` = (m0, m1, m2) trilinearly with align_corners, so native index i_a sits at grid coordinate
 * (i_a + p_a) (m_a - 1) / (P_a - 1) and a normalised displacement u_a is u_a (P_a - 1) / 2 padded native voxels.
 *  - irs_native_warp: per chain and native voxel, grid_sample (border, align_corners) of the PADDED native volume at identity +
 *    the displacement resized trilinearly (align_corners) from `dims` to P, cropped to the native box; the pad holds `fill`
 *    for the image and 0 for the segmentation and the mask.  Neither the padded volumes nor the resized field are ever
 *    formed: one launch walks the native grid, interpolates the three channels of the displacement at the voxel's grid
 *    coordinate, forms the source position r_a = (i_a + p_a) + u_a (P_a - 1) / 2 (one product, one sum: a zero displacement
 *    returns the moving volumes bit for bit), clamps it to [0, P_a - 1] and reads the taps from the unpadded volumes, a tap
 *    outside the native box being the fill.  displacement (C,3,m0,m1,m2) float32 in [-1,1] coordinates, channel 0 the last
 *    axis; C in 1 .. IRS_MAX_CHAINS; native: every n_a >= 1, fewer than 2^30 voxels; padding: every p_a >= 0; P_a >= 2; dims:
 *    every m_a >= 2.  im float32 / seg int16 / mask uint8: (Cim,1,n0,n1,n2) with Cim 1 (shared by the chains) or C, each
 *    NULL when its output is.  im_out float32 (trilinear) / seg_out int16 / mask_out uint8 (nearest, half to even as
 *    irs_warp_nearest_*): (C,1,n0,n1,n2) or NULL.  displacement_out (C,3,n0,n1,n2) float32 or NULL: the interpolated
 *    displacement times scale[c], three finite host floats, one per channel ((P_a - 1) / 2 of the channel's axis for native
 *    voxels, times the zoom for mm; NULL with a NULL output).  fill: finite.  At least one output must be asked for.
 *    Deterministic; no atomics; no host sync. */
int irs_native_warp(const float* displacement, int C, const int32_t* dims, const int32_t* native, const int32_t* padding,
                    const float* im, const int16_t* seg, const uint8_t* mask, int Cim, float fill, const float* scale,
                    float* im_out, int16_t* seg_out, uint8_t* mask_out, float* displacement_out, void* stream);

/* Native-grid posteriors (absent in the reference): the posterior label maps and the image posterior above, accumulated on the
 * image's own voxel grid in one fused launch per recorded step -- up-sample, warp and fold, with no warped volume in between.
 * The geometry (dims, native, padding), displacement, im, seg, Cim and fill are irs_native_warp's, with every n_a >= 2 in
 * addition (the finalizers need it).  Per chain c = 0 .. C-1, in order, and per native voxel the source position is formed once;
 *  - labels: the label is the value irs_native_warp writes to seg_out (nearest, half to even, 0 outside the native box);
 *    structure j is label value labels[j] as in irs_label_posterior_update (HOST int32, K in 1 .. IRS_MAX_LABELS, distinct, in
 *    the int16 range; every other value is "other").  counts (K,n0,n1,n2) int32, += 1 where the record carries the structure;
 *    volume (K,2) double {mean, M2}: Welford state of the per-record volumes (native voxels carrying the structure), folded with
 *    k = records_before + c + 1 (k = 1 overwrites it) -- the semantics of irs_label_posterior_update.
 *  - image: the sample x is bit for bit the value irs_native_warp writes to im_out.  mean, m2, low, high (n0,n1,n2) float32,
 *    updated in place with the recurrence of irs_image_posterior_update, k = records_before + c + 1: d = x - mean,
 *    mean += d / (float)k, m2 += d * (x - mean), low = fminf(low, x), high = fmaxf(high, x), every operation rounded to nearest
 *    on its own (no fused multiply-add); k = 1 overwrites the state (mean = low = high = x, m2 = 0), which is then never read.
 *  seg, labels, counts and volume are all given or all NULL, and so are im, mean, m2, low and high; at least one group must be
 *  given.  records_before >= 0, records_before + C <= INT32_MAX.  fill: finite.  ws: device workspace of
 *  irs_native_posterior_workspace bytes (K = 0 without the labels; never 0 bytes).  A thread owns a voxel: plain read-modify-
 *  writes, the state of the image in registers over the chains; exact integer sums in fixed order; two identical call sequences
 *  give identical bits; no host sync.  Both states go to irs_label_posterior_finalize / irs_image_posterior_finalize as they
 *  are, with (D,H,W) = native. */
int irs_native_posterior_workspace(int C, int K, const int32_t* native, size_t* bytes);
int irs_native_posterior_update(const float* displacement, int C, const int32_t* dims, const int32_t* native, const int32_t* padding,
                                const float* im, const int16_t* seg, int Cim, float fill, const int32_t* labels, int K,
                                int32_t* counts, double* volume, float* mean, float* m2, float* low, float* high,
                                int records_before, void* ws, size_t ws_bytes, void* stream);

/* Intensity similarity (absent in the reference, which reports only its loss terms and segmentation metrics): per chain the
 * joint intensity histogram of the fixed image and a (warped) moving image and, from ONE pass over the two volumes, MSE, the
 * global normalised cross-correlation, mutual information and normalised mutual information.
 *  - fixed (Cf,1,D,H,W) float32 with Cf 1 (shared by the chains) or C; moving (C,1,D,H,W) float32, C in 1 .. IRS_MAX_CHAINS;
 *    mask (1,1,D,H,W) uint8 shared by the chains, or NULL; every dim >= 1, fewer than 2^30 voxels.  A voxel takes part when
 *    the mask is set there (or is NULL) and both intensities are finite; masked voxels with a non-finite intensity are only
 *    counted (n_nonfinite).
 *  - binning, in float32: inv_w = (float)bins / (hi - lo) on the host, t = (x - lo) * inv_w (a difference, then a product),
 *    b = min(bins - 1, max(0, (int)floorf(t))); bins in IRS_SIMILARITY_MIN_BINS .. IRS_SIMILARITY_MAX_BINS; both ranges finite
 *    with hi > lo.  Values outside [lo, hi] fall into the end bins and the voxel is counted in n_clipped; x == hi is in bin
 *    bins - 1 and not clipped.
 *  - hist (C,bins,bins) int32 or NULL (the workspace then holds it): hist[c][bf][bm] over the voxels of chain c taking part.
 *    Exact: integer adds only.
 *  - stats (C, IRS_SIMILARITY_STATS) double: n, n_nonfinite, n_clipped, mse, ncc, h_fixed, h_moving, h_joint, mi, nmi.
 *    Entropies in nats from the counts, p = count / n: h_joint = -sum p ln p over the non-empty cells, h_fixed / h_moving the
 *    same over the row / column sums; mi = h_fixed + h_moving - h_joint; nmi = (h_fixed + h_moving) / h_joint (Studholme), NaN
 *    when h_joint == 0.  mse = sum (f - m)^2 / n with the difference formed in double.  ncc = (sum fm / n - mean_f mean_m) /
 *    sqrt(var_f var_m) from the raw double sums, NaN when a variance is <= 0.  n == 0: a zero histogram, NaN from mse on.
 *  - ws: irs_image_similarity_workspace(C, bins) bytes of device memory, 16-byte aligned (at most IRS_SIMILARITY_WS_BYTES).
 *  Deterministic (integer histogram, double sums merged in a fixed order); no host sync. */
#define IRS_SIMILARITY_STATS 10
#define IRS_SIMILARITY_MIN_BINS 2
#define IRS_SIMILARITY_MAX_BINS 128
#define IRS_SIMILARITY_MAX_BLOCKS 1024 /* rows of per-block partial sums in the workspace */
#define IRS_SIMILARITY_WS_BYTES \
    (IRS_MAX_CHAINS * IRS_SIMILARITY_MAX_BINS * IRS_SIMILARITY_MAX_BINS * 4 + IRS_SIMILARITY_MAX_BLOCKS * (3 + 6) * 8)
int irs_image_similarity_workspace(int C, int bins, size_t* bytes);
int irs_image_similarity(const float* fixed, int Cf, const float* moving, int C, const uint8_t* mask, int D, int H, int W,
                         float f_lo, float f_hi, float m_lo, float m_hi, int bins, int32_t* hist, double* stats, void* ws,
                         size_t ws_bytes, void* stream);

/* Local similarity maps (absent in the reference, whose only windowed quantity is the LCC normalisation inside its data
 * term): where the fixed image and a (warped) moving image agree -- the local normalised cross-correlation (LNCC) and SSIM
 * of every voxel's box window, their masked statistics, and the per-voxel posterior of the LNCC maps.
 *  - irs_local_similarity.  Inputs: fixed (Cf,1,D,H,W) float32 with Cf 1 (shared by the chains) or C; moving (C,1,D,H,W)
 *    float32, C in 1 .. IRS_MAX_CHAINS; mask (1,1,D,H,W) uint8 or NULL; every dim >= 1, fewer than 2^30 voxels; radius r in
 *    1 .. IRS_LOCAL_MAX_RADIUS; four host doubles floor_f, floor_m, c1, c2, each finite and > 0.
 *    Window: the (2r+1)^3 box around the voxel with every index clamped to the volume (replicate padding, the rule of the
 *    reference's LCC convolutions), so n = (2r+1)^3 is the same for every voxel.  The mask plays no part in the window; it
 *    only selects which voxels enter the statistics.
 *    Window sums: for each voxel and chain the five sums S_f, S_m, S_ff, S_mm, S_fm over the window are formed in float64,
 *    each float32 value converted to float64 first, so every product is exact.  mu_x = S_x / n, var_x = max(S_xx / n -
 *    mu_x^2, 0), cov = S_fm / n - mu_f mu_m.
 *    LNCC = clamp(cov / sqrt(var_f var_m), -1, 1) when var_f > floor_f and var_m > floor_m; otherwise the voxel is flat and
 *    its LNCC is NaN.  SSIM = ((2 mu_f mu_m + c1)(2 cov + c2)) / ((mu_f^2 + mu_m^2 + c1)(var_f + var_m + c2)), defined at
 *    flat voxels too.  A window holding any non-finite value of either image gives NaN in both maps at that voxel and
 *    affects no other voxel.
 *    Maps: lncc, ssim (C,1,D,H,W) float32; either may be NULL, and both when only the statistics are wanted.  Each stored
 *    value is the float64 value rounded once to float32.  Maps are written at every voxel, masked or not.
 *    stats (C, IRS_LOCAL_STATS) double: n, n_flat, n_nonfinite, lncc_mean, lncc_min, ssim_mean, ssim_min.  n counts the voxels
 *    of the mask (all voxels when it is NULL) whose window is finite, n_nonfinite those whose window is not, n_flat the flat
 *    ones among n.  The LNCC columns run over the n - n_flat defined voxels, the SSIM columns over the n voxels, all from the
 *    float64 values before rounding.  A mean over nothing is NaN, a minimum over nothing +inf.
 *    ws: IRS_LOCAL_WS_BYTES of device memory.  One launch for all chains and the second-stage reduction.  Deterministic: two
 *    identical calls are bit-identical and chain c of a C-chain call is bit-identical to the single-chain call on that
 *    chain's volumes (no float atomics, fixed-order sums, grids that depend on (D,H,W,C,r) only); no host sync.
 *  - irs_local_similarity_update: lncc (C,1,D,H,W) float32, C in 1 .. IRS_MAX_CHAINS, every dim >= 1; the per-voxel state mean,
 *    low (D,H,W) float32 and count (D,H,W) int32 (12 bytes per voxel), updated in place.  Per voxel the chains are folded in
 *    order and a NaN sample is skipped: k = ++count, mean = mean + (x - mean) / (float)k, low = fminf(low, x), every operation
 *    rounded once to float32.  records_before >= 0, records_before + C <= INT32_MAX; records_before = 0 overwrites the state
 *    (count 0, mean 0, low +inf before the first sample), which is then never read.  Each thread owns its voxels, no atomics;
 *    no host sync.
 *  - irs_local_similarity_finalize: the summary of the state over the mask ((D,H,W) uint8, or NULL: the whole volume).
 *    isummary: IRS_LOCAL_MAP_SUMMARY_INTS int64 {voxels, voxels with count == 0}; fsummary: IRS_LOCAL_MAP_SUMMARY_FLOATS
 *    doubles over the voxels with count > 0 {sum of mean, min of mean, min of low}; a minimum nothing entered is +inf.  ws:
 *    IRS_LOCAL_MAP_WS_BYTES of device memory.  Deterministic; no host sync. */
#define IRS_LOCAL_MAX_RADIUS 4
#define IRS_LOCAL_STATS 7
#define IRS_LOCAL_MAX_BLOCKS 1024 /* rows of per-block partial statistics per chain in the workspace */
#define IRS_LOCAL_WS_BYTES (IRS_MAX_CHAINS * IRS_LOCAL_MAX_BLOCKS * IRS_LOCAL_STATS * 8)
#define IRS_LOCAL_MAP_SUMMARY_INTS 2
#define IRS_LOCAL_MAP_SUMMARY_FLOATS 3
#define IRS_LOCAL_MAP_WS_BYTES (1024 * (IRS_LOCAL_MAP_SUMMARY_INTS + IRS_LOCAL_MAP_SUMMARY_FLOATS) * 8)
int irs_local_similarity(const float* fixed, int Cf, const float* moving, int C, const uint8_t* mask, int D, int H, int W,
                         int radius, double floor_f, double floor_m, double c1, double c2, float* lncc, float* ssim,
                         double* stats, void* ws, size_t ws_bytes, void* stream);
int irs_local_similarity_update(const float* lncc, int C, int D, int H, int W, float* mean, float* low, int32_t* count,
                                int records_before, void* stream);
int irs_local_similarity_finalize(const float* mean, const float* low, const int32_t* count, const uint8_t* mask, int D, int H,
                                  int W, long long* isummary, double* fsummary, void* ws, size_t ws_bytes, void* stream);

/* Residual model check (the numbers behind the reference's log_hist_res figure, logger/visualization.py:64-86): the data term
 * models the residual z as a zero-mean Gaussian mixture; these operators say whether that mixture fits the residuals it is
 * applied to -- the histogram and the moments of z, to be set against the mixture on the host -- and where it does not: the
 * per-voxel posterior mean of the negative log-likelihood.
 *  - irs_residual_histogram.  residuals (C,1,D,H,W) float32, C in 1 .. IRS_MAX_CHAINS; mask (1,1,D,H,W) uint8 shared by the
 *    chains, or NULL; every dim >= 1, fewer than 2^30 voxels; half_range h float32, finite and > 0; bins B in
 *    IRS_RESIDUAL_MIN_BINS .. IRS_RESIDUAL_MAX_BINS.  A voxel takes part when the mask is set there (or is NULL) and z is
 *    finite; masked voxels with a non-finite z are only counted (n_nonfinite).
 *    Binning, in float32: inv_w = (float)B / (2 * h) on the host, t = (z + h) * inv_w (a sum, then a product), b = min(B - 1,
 *    max(0, (int)floorf(t))).  |z| > h falls into the end bin and the voxel is counted in n_clipped; z == h is in bin B - 1
 *    and not clipped.
 *    hist (C,B) int64: hist[c][b] over the voxels of chain c taking part.  counts (C,3) int64: {n, n_nonfinite, n_clipped}.
 *    sums (C,4) double over the voxels taking part: {sum z, sum z^2, sum z^4, max |z|}, each z converted to double first (a
 *    maximum nothing entered is -inf).  The three arrays accumulate over calls: records_before == 0 overwrites them;
 *    otherwise (records_before > 0, records_before + C <= INT32_MAX) the call's integers are added, each of its three sums is
 *    added with one double add, and the maximum is merged.
 *    ws: IRS_RESIDUAL_WS_BYTES of device memory.  One launch for all chains and one finish launch.  Deterministic: two identical
 *    call sequences are bit-identical and chain c of a C-chain call is bit-identical to the single-chain call on that chain
 *    (integer atomics only, fixed-order double sums, a grid per chain that depends on the volume only); no host sync.
 *  - irs_residual_nll_update: residuals (C,1,D,H,W) float32, C in 1 .. IRS_MAX_CHAINS, every dim >= 1, fewer than 2^30 voxels.
 *    The model is two host arrays of K doubles, K in 1 .. IRS_MAX_COMPONENTS: log_weight[k] = ln pi_k - ln sigma_k - 1/2 ln 2 pi
 *    and inv_std[k] = 1 / sigma_k, every entry finite and inv_std > 0.  The per-voxel state mean (D,H,W) float32 and count
 *    (D,H,W) int32 (8 bytes per voxel) is updated in place.  Per voxel the chains are folded in order and a non-finite z is
 *    skipped; in float64 a_k = log_weight[k] - 1/2 (z inv_std[k])^2, m = max_k a_k, nll = -(m + log sum_k exp(a_k - m)),
 *    rounded once to float32; then k = ++count, mean = mean + (nll - mean) / (float)k, every operation rounded once to
 *    float32.  records_before >= 0, records_before + C <= INT32_MAX; records_before = 0 overwrites the state (count 0, mean
 *    0 before the first sample), which is then never read.  The map is written at every voxel, masked or not.  Each thread
 *    owns its voxels, no atomics; no host sync.
 *  - irs_residual_nll_finalize: the summary of the state over the mask ((D,H,W) uint8, or NULL: the whole volume).
 *    isummary: IRS_RESIDUAL_MAP_SUMMARY_INTS int64 {voxels, voxels with count == 0}; fsummary:
 *    IRS_RESIDUAL_MAP_SUMMARY_FLOATS doubles over the voxels with count > 0 {sum of mean, max of mean}; a maximum nothing
 *    entered is -inf.  ws: IRS_RESIDUAL_MAP_WS_BYTES of device memory.  Deterministic; no host sync. */
#define IRS_RESIDUAL_MIN_BINS 2
#define IRS_RESIDUAL_MAX_BINS 512
#define IRS_RESIDUAL_MAX_BLOCKS 1024 /* rows of per-block partial sums per chain in the workspace */
#define IRS_RESIDUAL_WS_BYTES (IRS_MAX_CHAINS * IRS_RESIDUAL_MAX_BLOCKS * (3 + 4) * 8)
#define IRS_RESIDUAL_MAP_SUMMARY_INTS 2
#define IRS_RESIDUAL_MAP_SUMMARY_FLOATS 2
#define IRS_RESIDUAL_MAP_WS_BYTES (1024 * (IRS_RESIDUAL_MAP_SUMMARY_INTS + IRS_RESIDUAL_MAP_SUMMARY_FLOATS) * 8)
int irs_residual_histogram(const float* residuals, int C, const uint8_t* mask, int D, int H, int W, float half_range, int bins,
                           long long* hist, long long* counts, double* sums, int records_before, void* ws, size_t ws_bytes,
                           void* stream);
int irs_residual_nll_update(const float* residuals, int C, int D, int H, int W, const double* log_weight, const double* inv_std,
                            int K, float* mean, int32_t* count, int records_before, void* stream);
int irs_residual_nll_finalize(const float* mean, const int32_t* count, const uint8_t* mask, int D, int H, int W,
                              long long* isummary, double* fsummary, void* ws, size_t ws_bytes, void* stream);

/* Coarse-to-fine start (absent in the reference, whose chains all start on the full grid): an image and a mask carried down to
 * a coarser grid and a field carried up to a finer one.  The grids are align_corners, as every resize of the package: along one
 * axis coarse index i of n sits at fine coordinate x_i = i (N - 1) / (n - 1) and fine index I of N at coarse coordinate
 * I (n - 1) / (N - 1), each formed in double as the integer product divided once.  A velocity or displacement in normalised
 * coordinates (2 spans n - 1 voxels) means the same on both grids and is not rescaled.  On every axis 2 <= n <= N; the fine
 * volume has fewer than 2^30 voxels; volumes times the first extent of the written grid is at most 65535 (one launch row each).
 * The sums are double, taken in the tap order z, then y, then x (acc = acc + ((w_z w_y) w_x) value, every operation rounded
 * once), and the result is rounded to float32 once.  Each is one launch with one thread per output element; deterministic; no
 * atomics; no host sync.
 *  - irs_restrict_image: im (Cim,1,D,H,W) float32 -> out (Cim,1,d,h,w), Cim >= 1.  A separable tent filter of half-width
 *    r = max(1, (N - 1) / (n - 1)) per axis: every integer k with |k - x_i| < r contributes the weight 1 - |k - x_i| / r to the
 *    fine voxel clamp(k, 0, N - 1) (replicate padding, as the Sobolev and the LNCC windows), and the weights of an axis are
 *    each divided by their sum (summed in the order of k).  n = N gives the identity bit for bit; N = 2 n - 1 gives the
 *    full-weighting stencil 1/4, 1/2, 1/4 (3/4, 1/4 at the two ends): all weights dyadic.
 *  - irs_restrict_mask: mask (Cm,1,D,H,W) uint8 -> out (Cm,1,d,h,w), Cm >= 1: the coarse voxel takes the fine voxel at
 *    floor(x_i + 0.5) per axis.
 *  - irs_prolong_field: x (C,ch,d,h,w) float32 -> out (C,ch,D,H,W), C >= 1, ch >= 1 (3 for a velocity, 1 for a scalar volume).
 *    Trilinear at the coarse coordinate c of every fine voxel: i0 = floor(c), weights 1 - (c - i0) and c - i0 on the taps i0 and
 *    i0 + 1.  Where i0 + 1 would be n its weight is 0 and the tap is not read.  n = N gives the identity bit for bit. */
int irs_restrict_image(const float* im, int Cim, int D, int H, int W, float* out, int d, int h, int w, void* stream);
int irs_restrict_mask(const uint8_t* mask, int Cm, int D, int H, int W, uint8_t* out, int d, int h, int w, void* stream);
int irs_prolong_field(const float* x, int C, int ch, int d, int h, int w, float* out, int D, int H, int W, void* stream);

/* Adaptive pSGLD preconditioner (absent in the reference, whose sigma field is the VI posterior's standard deviation): the diagonal
 * RMSprop estimator of Li et al. 2016 -- a running second moment of the gradient, and the sigma field formed from it.  All fields
 * live on the velocity grid (., 3, D, H, W) of the caller (the image grid for SVF_3D, the control grid for SVFFD_3D); every extent
 * >= 1, n = D H W < 2^30, ceil(H / 8) and 3 ceil(D / 4) at most 65535.  C in 1 .. IRS_MAX_CHAINS.  Every float32 operation named
 * below is one IEEE operation rounded to nearest (add, multiply, divide, square root); NO operation is fused: where a product is
 * added to something, the product is rounded first.  Doubles are used for the sums named so and nowhere else.
 *  - irs_precond_accumulate: grad_v (C,3,D,H,W) float32 as irs_io.grad_v hands it out (sigma^2 dL/dv_s), sigma (C,3,D,H,W) float32
 *    or NULL (= 1), beta in [0, 1), V (1,3,D,H,W) float32 in/out: ONE second moment shared by the chains.  Per element, float32:
 *    g_c = grad_v_c / (sigma_c sigma_c) (grad_v_c itself when sigma is NULL; sigma = 1 gives the same bits); q = g_0 g_0, then
 *    q = q + g_c g_c for c = 1 .. C - 1; m = q / (float)C; V = (beta V) + ((1 - beta) m) with 1 - beta one float32 subtraction.
 *    nonfinite: one int64 on the device, to which the number of non-finite g_c of the call is added (integer atomics, one per
 *    block that saw any); a non-finite g_c enters V like any other value.  V must not overlap grad_v or sigma.  One launch for
 *    all chains: 16-byte accesses when every array is 16-byte aligned and C = 1 or 3 n is a multiple of 4 (the rest of 3 n mod 4
 *    elements one by one), one element per thread otherwise; every thread owns its elements; no host sync.
 *  - irs_precond_sigma: V as above -> sigma (C,3,D,H,W) float32, the same field written to every chain, and summary,
 *    IRS_PRECOND_SUMMARY doubles on the device.  bias: 1 / (1 - beta^t) after t updates, formed by the caller in double, finite and
 *    >= 1; smooth r in 0 .. IRS_PRECOND_MAX_SMOOTH; damping > 0 and finite; 0 < sigma_min <= 1 <= sigma_max < inf.
 *    1. vhat = V (float)bias.  2. r > 0: every channel's vhat is replaced by its (2r+1)^3 box mean with replicate padding -- the
 *    window summed in double in the order dz, dy, dx ascending, divided by (2r+1)^3 in double, rounded to float32 once.
 *    3. s = sqrtf(vhat); sbar = (double sum of s over all N = 3 n elements) / N; lambda = (float)(damping sbar).
 *    4. G = 1 / (lambda + s); Gbar = (double sum of G) / N.  sbar == 0 (no gradient seen yet): G = 1 everywhere.
 *    5. raw = sqrtf(G / (float)Gbar); sigma = min(max(raw, sigma_min), sigma_max).
 *    The double sums are taken in a fixed order (per-thread strided sums, the lanes of a wavefront by a butterfly, the wavefronts
 *    and then the blocks in order; the grids depend on N only): two identical call sequences are bit-identical.
 *    summary: {sbar, Gbar, min sigma, max sigma, mean of sigma^2 (double products, double sum, / N), elements with raw <
 *    sigma_min, elements with raw > sigma_max, *nonfinite (the counter of irs_precond_accumulate, copied; NULL: 0)}.
 *    sigma must not overlap V.  ws: irs_precond_workspace bytes of device memory.  No atomics; no host sync.
 *  - irs_precond_workspace: the bytes irs_precond_sigma needs for the grid and r (a smoothed copy of vhat when r > 0, and the
 *    rows of per-block partial sums). */
#define IRS_PRECOND_MAX_SMOOTH 2
#define IRS_PRECOND_SUMMARY 8
int irs_precond_workspace(int D, int H, int W, int smooth, size_t* bytes);
int irs_precond_accumulate(const float* grad_v, const float* sigma, int C, int D, int H, int W, float beta, float* V,
                           long long* nonfinite, void* stream);
int irs_precond_sigma(const float* V, int C, int D, int H, int W, double bias, int smooth, double damping, float sigma_min,
                      float sigma_max, const long long* nonfinite, float* sigma, double* summary, void* ws, size_t ws_bytes,
                      void* stream);

/* Posterior principal modes (absent in the reference): the recorded displacements kept on the device and the Gram matrix the
 * snapshot PCA of them needs.  store (cap,3,D,H,W) float32, cap in 1 .. IRS_MODES_MAX_RECORDS, record i in slot i; every extent
 * >= 1, V = D H W < 2^30.  The host algebra (centring, the voxel scale, the eigen-decomposition) is the caller's.
 *  - irs_modes_gram_rows: one call per recorded step.  The n_new in 1 .. IRS_MAX_CHAINS new records are already in slots
 *    n_before .. n_before + n_new - 1, n_before >= 0, n_before + n_new <= cap; mask (D,H,W) uint8 (a voxel counts where != 0)
 *    or NULL (every voxel); gram (3,cap,cap) float64 in/out.  For every new slot i, every slot j <= i and every channel c:
 *    G[c][i][j] = sum over the voxels x the mask admits of (double)store[i][c][x] (double)store[j][c][x], and G[c][j][i] is
 *    written from the same value (the two triangles are bit-equal); no other element is touched.  Every product is exact in
 *    double (two 24-bit significands); the sums are double.  A voxel outside the mask is not read into any sum; a non-finite
 *    value inside it propagates.  Order of a sum: the voxels are dealt to B = min(256, ceil(V / 256)) blocks of 256 threads,
 *    thread t of block b adds its voxels b 256 + t, b 256 + t + 256 B, ... in order; the 64 lanes of a wavefront are added by
 *    the shuffle butterfly (offsets 32, 16, ..., 1), the four wavefronts in order, then the B blocks in order.  The order
 *    depends on V and these constants only -- not on n_before, n_new, cap or timing: the same records give the same bits, and
 *    an element has the same bits whichever call wrote it.  No atomics; two launches; no host sync.
 *    ws: irs_modes_gram_workspace bytes of device memory, 8-byte aligned (the rows of per-block partial sums).
 *  - irs_modes_gram_workspace: the bytes irs_modes_gram_rows needs for the grid and n_new, whatever n_before and cap.
 *  - irs_modes_project: the first n in 1 .. IRS_MODES_MAX_RECORDS slots of the store, coeff (M,n) float64 on the device, M in
 *    1 .. IRS_MODES_MAX, scale: three host doubles, finite and > 0 -> mean (3,D,H,W), modes (M,3,D,H,W), explained (D,H,W)
 *    float32.  Per voxel x and channel c, with x_i = (double)store[i][c][x], in record order i = 0 .. n - 1 from zero:
 *    S = S + x_i; Q = Q + x_i x_i (the product exact); a_m = a_m + (coeff[m][i] x_i) with the product rounded to double first
 *    and the sum rounded second -- never one fused operation.  mean[c][x] = (float)(S / n); modes[m][c][x] = (float)a_m.
 *    var_c = (Q - (S S) / n) / (n - 1), every operation rounded once.  explained[x] = (float)(num / den) with num = sum over c of
 *    scale_c^2 (sum over m of a_m a_m) on the unrounded a_m and den = sum over c of scale_c^2 var_c; 0 where den == 0 and for
 *    n < 2; no clamp (arbitrary coefficients may exceed 1); the mask plays no part.  Non-finite inputs propagate.  One launch,
 *    one voxel per thread, the channels one after the other; deterministic; no atomics; no host sync. */
#define IRS_MODES_MAX 16
#define IRS_MODES_MAX_RECORDS 1024
int irs_modes_gram_workspace(int D, int H, int W, int n_new, size_t* bytes);
int irs_modes_gram_rows(const float* store, int cap, int n_before, int n_new, int D, int H, int W, const uint8_t* mask, double* gram,
                        void* ws, size_t ws_bytes, void* stream);
int irs_modes_project(const float* store, int n, int D, int H, int W, const double* coeff, int M, const double* scale, float* mean,
                      float* modes, float* explained, void* stream);

/* Affine pre-alignment (absent in the reference, whose volumes were registered affinely elsewhere): the Gauss-Newton normal
 * equations of the sum of squared differences under a 3 x 4 map, the map as a transformation tensor, and the map composed with
 * a sampled transformation.
 * Voxel index coordinates in array order (D, H, W): index k = (k0, k1, k2), centre c = ((D - 1) / 2, (H - 1) / 2, (W - 1) / 2);
 * fixed and moving volume have the same extents, every one >= 2, fewer than 2^30 voxels.  A map is lin[9] (3 x 3, row-major) and
 * shift[3], host doubles, all finite.  Fixed voxel k reads the moving image at p = c + shift + lin (k - c), formed in double with
 * every operation rounded once and none contracted: p_a = (((lin[a][0] d_0 + lin[a][1] d_1) + lin[a][2] d_2) + shift[a]) + c_a,
 * d = k - c.  The identity gives p = k exactly.
 *  - irs_affine_normal_equations: fixed, moving (D,H,W) float32; mask (D,H,W) uint8 or NULL.  A voxel takes part when the mask
 *    is set (or absent), 0 <= p_a <= n_a - 1 on all three axes, and the fixed value and all eight moving taps are finite; the
 *    tests are made in that order (a masked voxel mapped outside counts as outside, whatever its values).  Cell i0 =
 *    min(floor(p), n - 2), w = p - i0 per axis.  The value M(p) and the gradient g = dM/dp (array order) are the trilinear
 *    interpolant's, in double from the float32 taps t: M = sum over the taps in the order z, y, x of ((wz wy) wx) t; g_0 = sum over
 *    (y, x) of (wy wx) (t[1][y][x] - t[0][y][x]), g_1 = sum over (z, x) of (wz wx) (t[z][1][x] - t[z][0][x]), g_2 = sum over (z, y)
 *    of (wz wy) (t[z][y][1] - t[z][y][0]); r = M(p) - F(k).  Parameters theta = (lin row-major, shift), 12; with kt = (d_0, d_1,
 *    d_2, 1): dr/dlin[a][b] = g_a kt_b, dr/dshift[a] = g_a.  H = sum J J^T with every term formed as (g_i g_j) (kt_a kt_b), b =
 *    sum J r with every term formed as (g_a r) kt_b.  sums (device, IRS_AFFINE_SUMS doubles): [0, 78) the upper triangle of H
 *    row-major, [78, 90) b, 90 sum r^2, 91 voxels taking part, 92 masked voxels mapped outside, 93 masked voxels inside dropped
 *    for a non-finite value (counts as doubles, exact).  ws: IRS_AFFINE_WS_BYTES, 8-byte aligned (IRS_AFFINE_MAX_BLOCKS rows of
 *    IRS_AFFINE_PARTIALS per-block sums, folded in a fixed order by a one-block kernel).  No floating-point atomics, a grid that
 *    depends on the extents only: two identical calls are bit-identical.  No host sync.
 *  - irs_affine_transformation: out (1,3,D,H,W) float32, the map as the [-1,1] transformation tensor the warps take
 *    (align_corners, component 0 = x, the last axis): 2 p_a / (n_a - 1) - 1 in double, rounded to float32 once.  D <= 65535.
 *  - irs_affine_compose: transformation (C,3,D,H,W) float32 in [-1,1], C in 1 .. IRS_MAX_CHAINS, C D <= 65535.  The moving image
 *    a chain saw after resampling through the map A is M'(y) = M(A y), so the total map is x -> A(phi(x)): every vector of phi
 *    goes to index coordinates ((g + 1) / 2) (n - 1) (in double, not clamped), through A as above with d = phi - c, and back.
 *    total_transformation (C,3,D,H,W) in [-1,1] and total_displacement (C,3,D,H,W) = A(phi(x)) - x in voxels, component 0 = x;
 *    either may be NULL, not both.  Element-wise, in double, rounded once. */
#define IRS_AFFINE_SUMS 94
#define IRS_AFFINE_PARTIALS 76        /* 60 distinct sums of H, 12 of b, sum r^2, three counts */
#define IRS_AFFINE_MAX_BLOCKS 512     /* rows of per-block partial sums in the workspace */
#define IRS_AFFINE_WS_BYTES (IRS_AFFINE_MAX_BLOCKS * IRS_AFFINE_PARTIALS * 8)
int irs_affine_normal_equations(const float* fixed, const float* moving, const uint8_t* mask, int D, int H, int W, const double* lin,
                                const double* shift, double* sums, void* ws, size_t ws_bytes, void* stream);
int irs_affine_transformation(const double* lin, const double* shift, float* out, int D, int H, int W, void* stream);
int irs_affine_compose(const float* transformation, const double* lin, const double* shift, float* total_transformation,
                       float* total_displacement, int C, int D, int H, int W, void* stream);

/* Cubic B-spline output resampling (absent in the reference, which resamples everything trilinearly): the interpolating cubic
 * B-spline of a volume, for the images that are written -- never for what the chain reads, whose adjoint is the trilinear one's.
 * A volume s of extents n = (D, H, W), every one >= 2 and fewer than 2^30 voxels, is extended by whole-sample mirroring
 * (k < 0 -> -k, k > n - 1 -> 2 (n - 1) - k; scipy's mode='mirror').
 *  - Coefficients (irs_bspline_prefilter): im (Cim,1,D,H,W) float32 -> coeff of the same shape, Cim in 1 .. IRS_MAX_CHAINS,
 *    Cim D <= 65535; coeff may be im.  The lines are filtered separably, along x (the last axis), then y, then z.  Per line of
 *    length n, with z1 = sqrt(3) - 2 and gain 6, in double, every operation rounded once and none contracted, T = 2 n - 2 and
 *    mir() the mirror above:
 *      1. c+[0] = (sum_{k=0}^{T-1} zk (6 s[mir(k)])) / (1 - z1^T) when T <= 32, otherwise the first 32 terms of the same series
 *         with no divisor (|z1|^32 / (1 - |z1|) = 7e-19 is below double rounding); the sum starts at 0 and runs in the order of
 *         k; zk starts at 1 and is multiplied by z1 after every term, and z1^T is zk after the last one;
 *      2. c+[k] = 6 s[k] + z1 c+[k-1] for k = 1 .. n - 1;
 *      3. c[n-1] = (z1 / (z1^2 - 1)) (c+[n-1] + z1 c+[n-2]), the constant formed on the host in double;
 *      4. c[k] = z1 (c[k+1] - c+[k]) for k = n - 2 .. 0.
 *    The running values -- c+[k-1] in 2, c[k+1] in 4 -- are carried in double.  The line rests in float32 between its two
 *    sweeps: every c+[k] is stored rounded to float32 once and steps 3 and 4 read the stored values (coeff may be the input and
 *    there is no workspace, so float32 is all there is); every c[k] is rounded to float32 once when it is stored, and the next
 *    axis reads float32.  Three launches; no scratch; deterministic; no atomics; no host sync.
 *  - Evaluation at a position q in index coordinates, in float32, every operation rounded once: per axis q is clamped to
 *    [0, n - 1] (the border rule of every warp; a NaN goes to 0), i0 = min(floor(q), n - 2), t = q - i0, u = 1 - t; the taps are
 *    i0 - 1 .. i0 + 2, mirrored once, with the weights w0 = u*u*u/6, w1 = (3*t*t*t - 6*t*t + 4)/6, w2 = (3*u*u*u - 6*u*u + 4)/6,
 *    w3 = t*t*t/6, each formed left to right as written.  The sum is separable: for every (z, y) tap pair the row sum over the
 *    four x taps, acc = acc + w c from 0 with the taps ascending; then the four row sums over y in the same way; then over z.
 *  - irs_bspline_warp, the twin of irs_warp_transformation: coeff (Cim,1,D,H,W) float32 with Cim 1 (shared) or C;
 *    transformation (C,3,D,H,W) float32 in [-1,1], component 0 = x; out (C,1,D,H,W): the spline at the index coordinate
 *    ((g + 1) * 0.5) * (n - 1) of every voxel, as the trilinear sampler forms it.  C in 1 .. IRS_MAX_CHAINS, C D <= 65535.  One
 *    launch, one thread per output voxel.
 *  - irs_native_warp_cubic, the image output of irs_native_warp with the cubic rule (labels and masks stay with that call):
 *    displacement, dims, native, padding, Cim, fill and im_out as there, every native extent >= 2; im (Cim,1,n0,n1,n2) the
 *    unpadded native image and coeff its irs_bspline_prefilter.  The source position r of a voxel is irs_native_warp's (the
 *    same expressions).  Where all eight trilinear taps of r lie inside the native box the value is the spline of the unpadded
 *    volume at q = r - p, from coeff; elsewhere -- in the pad and on the ramp between the image edge and the fill -- it is the
 *    trilinear blend with `fill` read from im, exactly what irs_native_warp writes.  One launch; deterministic; no host sync. */
int irs_bspline_prefilter(const float* im, float* coeff, int Cim, int D, int H, int W, void* stream);
int irs_bspline_warp(const float* coeff, int Cim, const float* transformation, float* out, int C, int D, int H, int W, void* stream);
int irs_native_warp_cubic(const float* displacement, int C, const int32_t* dims, const int32_t* native, const int32_t* padding,
                          const float* im, const float* coeff, int Cim, float fill, float* im_out, void* stream);

/* Foreground masks from the image (absent in the reference, which reads every mask from a file): histogram, connected components,
 * selection of the largest components, hole filling and ball morphology.  Every call takes C >= 1 volumes (C,1,D,H,W), every
 * extent >= 1, fewer than 2^30 voxels each and C D <= 65535, and treats the volumes independently; a mask is uint8, set where
 * non-zero, and every mask written holds 0 / 1.  Nothing is a neighbour across the end of a row, a plane or a volume.  Every
 * result is a function of the input alone (integer counts, canonical labels): atomics are used and two calls are still
 * bit-identical.  No call synchronises with the host.
 *  - irs_intensity_histogram: im (C,1,D,H,W) float32; mask (Cm,1,D,H,W) with Cm 1 (shared) or C, or NULL; lo < hi finite; bins in
 *    IRS_MASK_MIN_BINS .. IRS_MASK_MAX_BINS; hist (C,bins) int64, overwritten.  A voxel counts when the mask is set (or absent) and
 *    its value is finite; its bin is that of irs_image_similarity: in float32, inv_w = bins / (hi - lo), t = (x - lo) * inv_w,
 *    b = min(bins - 1, max(0, floor(t))), so a value outside [lo, hi] lands in the first or the last bin.  One launch.
 *  - irs_mask_threshold: out = im > threshold (a NaN is background).
 *  - irs_connected_components: connectivity 6, 18 or 26 (neighbours that differ in at most 1, 2 or 3 coordinates, by one each);
 *    labels (C,1,D,H,W) int32: 0 background, the components of each volume numbered 1 .. n in ascending order of their smallest
 *    linear voxel index; counts (C) int32: n.  ws: irs_connected_components_workspace bytes (two int32 fields and one int32 per
 *    1024 voxels), 16-byte aligned.  Six launches: union-find in LDS tiles, unions across tile faces, flatten, scan of the root
 *    counts, root numbers, relabel; every loop has a trip bound that follows from the voxel count and no workgroup waits for another.
 *  - irs_mask_keep_largest: out = the voxels of the `keep` (1 .. IRS_MASK_MAX_KEEP) largest components of each volume, ties going
 *    to the smaller number; fewer components: all of them; an empty mask stays empty.  irs_mask_fill_holes: out = mask, plus the
 *    background voxels with no 6-connected background path to the border of the volume (scipy's binary_fill_holes with its default
 *    structure).  ws of both: irs_mask_select_workspace bytes, 16-byte aligned; out may be mask.
 *  - irs_mask_dilate: out = the voxels whose squared distance, in voxels, to the nearest set voxel is <= r2, 0 <= r2 <=
 *    IRS_MASK_MAX_RADIUS^2: the dilation by the Euclidean ball, compared in integers.  erode != 0: the same for the complement,
 *    complemented -- the erosion; voxels outside the volume are not background, so a mask on the border is not eaten from there.
 *    ws: irs_mask_morphology_workspace bytes (3 bytes per voxel), 16-byte aligned; out may be mask.  Three launches. */
#define IRS_MASK_MIN_BINS 2
#define IRS_MASK_MAX_BINS 4096
#define IRS_MASK_MAX_KEEP 64
#define IRS_MASK_MAX_RADIUS 16
int irs_intensity_histogram(const float* im, int C, const uint8_t* mask, int Cm, int D, int H, int W, float lo, float hi, int bins,
                            long long* hist, void* stream);
int irs_mask_threshold(const float* im, int C, int D, int H, int W, float threshold, uint8_t* out, void* stream);
int irs_connected_components_workspace(int C, int D, int H, int W, size_t* bytes);
int irs_connected_components(const uint8_t* mask, int C, int D, int H, int W, int connectivity, int32_t* labels, int32_t* counts,
                             void* ws, size_t ws_bytes, void* stream);
int irs_mask_select_workspace(int C, int D, int H, int W, size_t* bytes);
int irs_mask_keep_largest(const uint8_t* mask, int C, int D, int H, int W, int connectivity, int keep, uint8_t* out, void* ws,
                          size_t ws_bytes, void* stream);
int irs_mask_fill_holes(const uint8_t* mask, int C, int D, int H, int W, uint8_t* out, void* ws, size_t ws_bytes, void* stream);
int irs_mask_morphology_workspace(int C, int D, int H, int W, size_t* bytes);
int irs_mask_dilate(const uint8_t* mask, int C, int D, int H, int W, int r2, int erode, uint8_t* out, void* ws, size_t ws_bytes,
                    void* stream);

/* Landmark propagation (absent in the reference, which has no point-set operator): a sampled displacement evaluated at K
 * positions that are no voxel centres, and the posterior of the mapped landmarks with their target registration error (TRE).
 * warped(x) = moving(x + d(x)): a point p of the fixed grid maps to p + d(p) in the moving image; points of the moving space
 * are carried to the fixed space with the displacement of irs_svf_exp_inverse.
 *  - irs_transform_points: points (K,3) float32 in [-1,1] coordinates (align_corners), component 0 = x (the last axis), K in
 *    1 .. IRS_LANDMARK_MAX_POINTS; displacement (C,3,D,H,W) float32 in any linear unit, channel 0 the last axis, C in 1 ..
 *    IRS_MAX_CHAINS, every dim >= 2; scale: 3 host floats, finite and > 0, one per channel; offset (K,3) float32 or NULL (= 0).
 *    sampled (C,K,3) float32 or NULL: the three channels sampled at the point with the trilinear sampler of the squaring step
 *    and the warp (border clamp, align_corners, the same expressions: index coordinate ((g + 1) * 0.5) * (n - 1), weights
 *    (wx * wy) * wz, acc = acc + val * w over the corners x fastest, every operation rounded once to float32), so a point on a
 *    voxel centre returns the stored value bit for bit and a point outside the box the border value.  mapped (C,K,3) float32
 *    or NULL: scale_c * sampled_c + offset_c, one product and one sum, each rounded once; with the point's position in the
 *    output unit as the offset this is the mapped point.  At least one of the two outputs must be given.  A point with a
 *    non-finite coordinate gives NaN in all three components of both outputs and reads no tap.  One launch, one thread per
 *    (chain, point); deterministic; no atomics; no host sync.
 *  - irs_landmark_update: mapped (C,K,3) and target (K,3) float32 in one common unit.  The state is float64: mean (K,3),
 *    comoment (K,6: xx, xy, xz, yy, yz, zz), tre_mean, tre_m2, tre_max (K), and count (K) int32.  Per landmark, the chains in
 *    order; a sample takes part when its three components and the landmark's target are finite (else it is skipped and not
 *    counted): k = ++count, delta = x - mean, mean += delta / k, comoment_ab += delta_a * (x_b - mean_b) with the new mean;
 *    e = sqrt(sum_c (x_c - target_c)^2) in double, folded into tre_mean / tre_m2 the same way, tre_max = fmax(tre_max, e).
 *    records_before >= 0 records were folded in before, records_before + C <= INT32_MAX; records_before = 0 overwrites the
 *    state (all zero before the first sample), which is then never read.  One launch, each thread owns its landmarks, no
 *    atomics.  Deterministic; no host sync.
 *  - irs_landmark_finalize: out (K, IRS_LANDMARK_COLUMNS) doubles per landmark {count, tre_mean, tre_std = sqrt(tre_m2 /
 *    max(count - 1, 1)), tre_max, tre_of_mean = |mean - target|, the three principal standard deviations of S = comoment /
 *    max(count - 1, 1), descending (the 5 cyclic Jacobi sweeps of irs_displacement_covariance_finalize, eigenvalues clamped at
 *    0 under the root), mahalanobis2 = sum_i ((mean - target) . e_i)^2 / l_i over the eigenpairs of S, pit = F3(mahalanobis2)
 *    with F3(x) = erf(sqrt(x / 2)) - sqrt(2 x / pi) exp(-x / 2), the chi-square CDF with 3 degrees of freedom}.  count == 0:
 *    every column but the first is NaN.  mahalanobis2 and pit are NaN when count < 4 or the smallest eigenvalue is <= 0.
 *    isummary: IRS_LANDMARK_SUMMARY_INTS int64 {landmarks, landmarks with count == 0, landmarks with a finite pit}; fsummary:
 *    IRS_LANDMARK_SUMMARY_FLOATS doubles over the landmarks with count > 0 {sum tre_of_mean, max tre_of_mean, sum tre_mean,
 *    max tre_max}; a maximum nothing entered is -inf.  ws: IRS_LANDMARK_WS_BYTES of device memory.  Deterministic (exact
 *    integer sums, fixed-order double sums and maxima); no host sync. */
#define IRS_LANDMARK_MAX_POINTS (1 << 24)
#define IRS_LANDMARK_COLUMNS 10
#define IRS_LANDMARK_SUMMARY_INTS 3
#define IRS_LANDMARK_SUMMARY_FLOATS 4
#define IRS_LANDMARK_WS_BYTES (1024 * (IRS_LANDMARK_SUMMARY_INTS + IRS_LANDMARK_SUMMARY_FLOATS) * 8)
int irs_transform_points(const float* points, int K, const float* displacement, int C, int D, int H, int W, const float* scale,
                         const float* offset, float* sampled, float* mapped, void* stream);
int irs_landmark_update(const float* mapped, const float* target, int C, int K, double* mean, double* comoment, double* tre_mean,
                        double* tre_m2, double* tre_max, int32_t* count, int records_before, void* stream);
int irs_landmark_finalize(const double* mean, const double* comoment, const double* tre_mean, const double* tre_m2,
                          const double* tre_max, const int32_t* count, const float* target, int K, double* out, long long* isummary,
                          double* fsummary, void* ws, size_t ws_bytes, void* stream);

/* Structure report (absent in the reference, whose every summary is one number over the mask): per structure of the fixed
 * segmentation, the sums behind the posterior of its mean displacement and of its volume change, reduced from ONE recorded
 * sample per row, and the same labelled reduction over finished per-voxel maps.  seg_fixed (D,H,W) int16 is shared by the rows;
 * structure j is label value labels[j] (HOST int32, n_labels = K in 1 .. IRS_MAX_LABELS, distinct, in the int16 range).  Voxel p
 * belongs to structure j when seg_fixed[p] == labels[j] and, with mask (D,H,W) uint8 given (NULL: none), mask[p] != 0; every
 * other value of the map -- 0, negative values and unlisted labels included -- belongs to no structure.
 *  - irs_structure_motion: displacement (C,3,D,H,W) float32 in voxels as the transition writes it, transformation (C,3,D,H,W)
 *    float32 in [-1,1] coordinates (required), C in 1 .. IRS_MAX_CHAINS, every dim >= 2 (det J reads a neighbour); scale: 3
 *    host floats, finite and > 0, one per channel.  Per (chain, structure), over the structure's voxels: ints (C,K,
 *    IRS_STRUCTURE_MOTION_INTS) int64 {voxels, folded}; floats (C,K,IRS_STRUCTURE_MOTION_FLOATS) doubles {sum w_x, sum w_y,
 *    sum w_z, sum |w|, sum |w|^2, max |w|, sum det J, min det J, max det J}.  w_c = (double)u_c * (double)scale_c (exact);
 *    |w|^2 = (w_x^2 + w_y^2) + w_z^2 and |w| = sqrt(|w|^2) in double, every operation rounded once.  det J is the float32 value
 *    irs_log_det_jacobian and irs_jacobian_posterior_update form (the same device function), converted to double; a voxel is
 *    folded when !(det > 0), NaN included, and a NaN det is left out of the three det columns (the columns do not tell how
 *    many were).  A non-finite displacement propagates into its structure's sums; the maximum drops a NaN, as fmax does.
 *  - irs_structure_map_stats: maps (M,D,H,W) float32, any M >= 1, every dim >= 1.  Per (map, structure): ints (M,K,
 *    IRS_STRUCTURE_MAP_INTS) int64 {finite, non_finite} values; floats (M,K,IRS_STRUCTURE_MAP_FLOATS) doubles {sum x, sum x^2,
 *    min, max} over the finite values, x^2 formed in double (exact).
 *  An empty structure gives integers 0 and sums 0.0; a maximum nothing entered stays -inf, a minimum +inf.  The output
 *  pointers are device arrays and may point into a larger series buffer.  ws: device workspace of irs_structure_workspace bytes,
 *  rows = C or M.  Two stages: per block of the stream, per wavefront and distinct structure a shuffle reduction into the
 *  wavefront's own table, the tables merged in order; then the blocks' partials folded in block order.  Sums in double in an
 *  order fixed by the shapes and the label map, no floating-point atomics, exact counts: two identical calls are bit-identical.
 *  A refused call writes nothing.  No host sync. */
#define IRS_STRUCTURE_MOTION_INTS 2
#define IRS_STRUCTURE_MOTION_FLOATS 9
#define IRS_STRUCTURE_MAP_INTS 2
#define IRS_STRUCTURE_MAP_FLOATS 4
int irs_structure_workspace(int D, int H, int W, int n_labels, int rows, size_t* bytes);
int irs_structure_motion(const float* displacement, const float* transformation, int C, int D, int H, int W, const int16_t* seg_fixed,
                         const int32_t* labels, int n_labels, const uint8_t* mask, const float* scale, long long* ints,
                         double* floats, void* ws, size_t ws_bytes, void* stream);
int irs_structure_map_stats(const float* maps, int M, int D, int H, int W, const int16_t* seg_fixed, const int32_t* labels,
                            int n_labels, const uint8_t* mask, long long* ints, double* floats, void* ws, size_t ws_bytes,
                            void* stream);

/* Known-transformation validation (absent in the reference): the recorded displacement against a dense truth t (3,D,H,W) float32
 * on the fixed grid, in the unit of the displacement.  scale: 3 HOST floats s, finite and > 0, one per channel; mask (D,H,W)
 * uint8 or NULL (whole volume).  All arithmetic below is in double, every operation rounded once, nothing contracted.
 *  - irs_truth_update: displacement (C,3,D,H,W) float32, C in 1 .. IRS_MAX_CHAINS, every dim >= 2; below (3,D,H,W) uint16,
 *    updated in place: below[c,x] += #{chains k: u_k,c(x) < t_c(x)}, the comparison strict and on the raw float32 values (false
 *    when either side is NaN), whatever the mask says.  records_before >= 0 records were counted before, records_before + C <=
 *    IRS_TRUTH_MAX_RECORDS; records_before = 0 overwrites below, which is then never read.  Per chain, over the masked voxels:
 *    e_c = s_c * ((double)u_c - (double)t_c), q = (e_x^2 + e_y^2) + e_z^2, r = sqrt(q); ints (C, IRS_TRUTH_UPDATE_INTS) int64
 *    {voxels, voxels with a non-finite q}; floats (C, IRS_TRUTH_UPDATE_FLOATS) doubles over the other masked voxels {sum r,
 *    sum q, max r}; a maximum nothing entered is -inf.  ints / floats are device pointers and may point into a larger series.
 *    ws: IRS_TRUTH_UPDATE_WS_BYTES of device memory.  One launch and one finish launch.
 *  - irs_truth_calibrate: mean (3,D,H,W), comoment (6,D,H,W: xx, yy, zz, xy, xz, yz) float32: a state of
 *    irs_displacement_covariance_update after n records, 2 <= n <= IRS_TRUTH_MAX_RECORDS; below: as above after the same n
 *    records; std_floor f, finite, > 0 and f^2 > 0.  Per voxel: Delta_c = s_c * ((double)mean_c - (double)t_c); A_ab = ((s_a *
 *    s_b) * (double)comoment_ab) / (double)(n - 1), and A_cc += f^2.  LDL^T without pivoting: d0 = A_xx; l10 = A_xy / d0, l20 =
 *    A_xz / d0; d1 = A_yy - l10 * A_xy; w = A_yz - l20 * A_xy, l21 = w / d1; d2 = (A_zz - l20 * A_xz) - l21 * w; every pivot is
 *    raised to f^2 the moment it is formed if it is below (or NaN) -- in exact arithmetic none is -- and a voxel with a raised
 *    pivot counts as `raised`.  y0 = Delta_x, y1 = Delta_y - l10 * y0, y2 = (Delta_z - l20 * y0) - l21 * y1; dist2 = (y0 * y0 /
 *    d0 + y1 * y1 / d1) + y2 * y2 / d2; err2 = (Delta_x^2 + Delta_y^2) + Delta_z^2; v = (A_xx + A_yy) + A_zz; z_c = Delta_c^2 /
 *    max(A_cc, f^2).  Maps (D,H,W) float32, whatever the mask says: error = (float)sqrt(err2), mahalanobis = (float)sqrt(dist2);
 *    a voxel with a non-finite value among its 12 state and truth values, or a non-finite dist2, is `non-finite`: NaN in both.
 *    Over the masked voxels that are not non-finite, exact int64 counts (IRS_TRUTH_COUNTS(B, L, Br) of them, in this order):
 *    pit_hist[B]: bin = number of d2_edges <= dist2 (B - 1 HOST doubles, finite and strictly increasing, B in 1 ..
 *    IRS_TRUTH_MAX_BINS); coverage[L]: dist2 <= levels[l] (L HOST doubles, finite, L in 1 .. IRS_TRUTH_MAX_LEVELS);
 *    rank_hist[3][Br]: bin = min(below_c * Br / (n + 1), Br - 1) in integers, Br in 1 .. IRS_TRUTH_MAX_BINS.  The reliability
 *    table over R in 1 .. IRS_TRUTH_MAX_RELIABILITY_BINS bins of v, bin = number of var_edges <= v (R - 1 HOST doubles, finite
 *    and strictly increasing): rel_ints (R) int64 {voxels}, rel_floats (R,2) doubles {sum v, sum err2}, by the labelled
 *    reduction of irs_structure_motion with the bin as the label.  isummary: IRS_TRUTH_SUMMARY_INTS int64 over the mask {voxels,
 *    non-finite voxels, raised voxels}; fsummary: IRS_TRUTH_SUMMARY_FLOATS doubles over the other masked voxels {sum
 *    sqrt(err2), sum err2, max sqrt(err2), sum dist2, max dist2, sum v, sum z_x, sum z_y, sum z_z}.  No transcendental is
 *    evaluated on the device: whatever needs a distribution function is decided against the thresholds the host passes.  ws:
 *    IRS_TRUTH_CALIBRATE_WS_BYTES of device memory.
 *  Both: the grids depend on the volume alone; the double sums are reduced in two stages with a fixed merge order and no
 *  floating-point atomics; the counts are integer sums.  Two identical calls are bit-identical.  A refused call writes nothing.
 *  No host sync. */
#define IRS_TRUTH_MAX_RECORDS 65535
#define IRS_TRUTH_UPDATE_INTS 2
#define IRS_TRUTH_UPDATE_FLOATS 3
#define IRS_TRUTH_UPDATE_WS_BYTES (IRS_MAX_CHAINS * 1024 * (IRS_TRUTH_UPDATE_INTS + IRS_TRUTH_UPDATE_FLOATS) * 8)
#define IRS_TRUTH_MAX_BINS 64
#define IRS_TRUTH_MAX_LEVELS 8
#define IRS_TRUTH_MAX_RELIABILITY_BINS 32
#define IRS_TRUTH_RELIABILITY_INTS 1
#define IRS_TRUTH_RELIABILITY_FLOATS 2
#define IRS_TRUTH_SUMMARY_INTS 3
#define IRS_TRUTH_SUMMARY_FLOATS 9
#define IRS_TRUTH_CALIBRATE_WS_BYTES \
    (1024 * (IRS_TRUTH_SUMMARY_INTS + IRS_TRUTH_SUMMARY_FLOATS + IRS_TRUTH_MAX_RELIABILITY_BINS * (IRS_TRUTH_RELIABILITY_INTS + IRS_TRUTH_RELIABILITY_FLOATS)) * 8)
#define IRS_TRUTH_COUNTS(B, L, Br) ((B) + (L) + 3 * (Br))
int irs_truth_update(const float* displacement, int C, int D, int H, int W, const float* truth, uint16_t* below, const uint8_t* mask,
                     const float* scale, int records_before, long long* ints, double* floats, void* ws, size_t ws_bytes,
                     void* stream);
int irs_truth_calibrate(const float* mean, const float* comoment, const uint16_t* below, const float* truth, int D, int H, int W, int n,
                        const float* scale, double std_floor, const uint8_t* mask, const double* d2_edges, int pit_bins,
                        const double* levels, int n_levels, int rank_bins, const double* var_edges, int reliability_bins,
                        float* error, float* mahalanobis, long long* counts, long long* rel_ints, double* rel_floats,
                        long long* isummary, double* fsummary, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fused transition (Trainer._SGLD_transition, trainer/trainer.py:291-356)
 * ---------------------------------------------------------------------------------------------- */

typedef struct irs_config {
    int32_t dims[3];        /* D, H, W of the images */
    int32_t cps[3];         /* control point spacing; all 0 -> SVF_3D, else SVFFD_3D */
    int32_t no_chains;      /* C */
    int32_t no_steps;       /* 12 */
    int32_t sobolev_s;      /* 0 -> disabled */
    float sobolev_kernel[2 * IRS_MAX_HALF_WIDTH + 1];
    float lr;               /* optimizer_SG_MCMC lr == tau (trainer.py:607) */
    float uniform_alpha;    /* <= 0 -> disabled */
    int32_t virtual_decimation;
    int32_t data_loss;      /* IRS_DATA_* */
    int32_t lcc_s;          /* IRS_DATA_LNCC: the window radius, 1 .. IRS_MAX_HALF_WIDTH (weight and eps: irs_lncc_set);
                             * IRS_DATA_MI: the bins, IRS_MI_MIN_BINS .. IRS_MI_MAX_BINS (weight and ranges: irs_mi_set); IRS_DATA_NGF: not read */
    int32_t gmm_components;
    float ssd_sigma;
    /* optimizer_GMM (optimizers/adam_rate_decay.py) + hyper-priors (trainer.py:68-77) */
    float gmm_lr_log_std, gmm_lr_logits, gmm_lr_decay;
    float adam_beta1, adam_beta2, adam_eps;
    float scale_prior_loc, scale_prior_scale;             /* LogScaleNormalPrior */
    float dirichlet_concentration[IRS_MAX_COMPONENTS];    /* DirichletPrior */
    /* regulariser (model/loss.py:172-312) */
    int32_t reg_loss;       /* IRS_REG_* */
    int32_t reg_learnable;
    float w_reg;
    double dof;             /* 3 * prod(image dims), parse_config.py:120,128 */
    float reg_lr0, reg_lr1, reg_lr_decay; /* (lr_loc, lr_log_scale) or (lr_log_w_reg, -) */
    float loc_prior_nu, loc_prior_w_reg;  /* LogEnergyExpGammaPrior */
    float reg_scale_prior_loc, reg_scale_prior_scale; /* LogScaleNormalPrior on log_scale */
    int32_t diff_op;        /* IRS_DIFF_*; 0 (a zeroed struct) is the GradientOperator.  Sits where the padding in front of
                               the doubles was: no other offset moved */
    double w_reg_prior_shape, w_reg_prior_rate;       /* LogPrecisionExpGammaPrior (learnable RegLoss_L2);
                                                         RegLoss_Student (model/loss.py:201-241): {a0, 2 b0} */
    uint64_t seed;          /* Philox key for in-kernel noise */
} irs_config;

/* hyper-parameter + optimiser state that lives on the device between transitions */
typedef struct irs_state {
    float gmm_log_std[IRS_MAX_COMPONENTS];
    float gmm_logits[IRS_MAX_COMPONENTS];
    double gmm_adam_m[2][IRS_MAX_COMPONENTS];
    double gmm_adam_v[2][IRS_MAX_COMPONENTS];
    int64_t gmm_adam_step[2];
    double reg_param[2];     /* L2: {log_w_reg, -}; LogNormal: {loc, log_scale} */
    double reg_adam_m[2], reg_adam_v[2];
    int64_t reg_adam_step[2];
    uint64_t iteration;      /* Philox counter, incremented by every transition */
} irs_state;

/* per-transition scalars (loss_terms / aux of the reference's return triple) */
typedef struct irs_scalars {
    double alpha[IRS_MAX_CHAINS];       /* VD factor */
    double data_term[IRS_MAX_CHAINS];   /* alpha * sum(-log p(z)) */
    double reg_term[IRS_MAX_CHAINS];
    double reg_energy[IRS_MAX_CHAINS];  /* y */
    double n_mask[IRS_MAX_CHAINS];
} irs_scalars;

typedef struct irs_io {
    const float* fixed_im;   /* (Cf,1,D,H,W) */
    const float* moving_im;  /* (Cm,1,D,H,W) */
    const uint8_t* mask;     /* (Cmask,1,D,H,W) */
    int32_t fixed_chains, moving_chains, mask_chains; /* 1 (shared) or C */
    float* v;                /* (C,3,Dv,Hv,Wv) in/out: v_curr_state */
    const float* sigma;      /* (C,3,Dv,Hv,Wv) or NULL (= 1) */
    const float* eps;        /* injected N(0,1) noise or NULL (Philox) */
    const float* unif;       /* injected U[0,1) noise (C,3,D,H,W) or NULL (Philox) */
    /* outputs (caller-owned; any may be NULL to skip) */
    float* curr_state;       /* (C,3,Dv,Hv,Wv) smoothed velocity = the recorded sample */
    float* im_moving_warped; /* (C,1,D,H,W) */
    float* residuals;        /* (C,1,D,H,W) dense z */
    float* displacement;     /* (C,3,D,H,W) voxels */
    float* transformation;   /* (C,3,D,H,W) [-1,1] */
    float* grad_v;           /* (C,3,Dv,Hv,Wv) v.grad of the reference: sigma^2 * dL/dv_s (debug / parity) */
} irs_io;

typedef struct irs_ctx irs_ctx;

/* allocates the workspace (saved scaling-and-squaring steps, gradients, tile scratch) with hipMalloc. blocking. */
int irs_create(const irs_config* cfg, irs_ctx** out);
void irs_destroy(irs_ctx* ctx);
size_t irs_workspace_bytes(const irs_ctx* ctx);
/* control-grid size for the configured transformation model (utils/util.py:61-69) */
int irs_velocity_dims(const irs_ctx* ctx, int32_t out[3]);

/* pre-normalise the fixed image for the LCC map (iteration-invariant half of model/loss.py:103-105). */
int irs_set_fixed(irs_ctx* ctx, const float* fixed_im, int fixed_chains, void* stream);
/* IRS_DATA_LNCC: the data term of a chain is weight * sum mask * d (irs_lncc_fwd, radius = irs_config.lcc_s), alpha[c] = 1, and
 * irs_io.residuals receives d at every voxel.  weight > 0, eps > 0, both finite; a context starts with 1 and 1e-5.  They travel
 * here because irs_config has no room left, and may be set only before the first transition.  Such a context takes no virtual
 * decimation and no z-slab, and its sparse data and sparse forward stages stay off (the sparse adjoint works as ever). */
int irs_lncc_set(irs_ctx* ctx, float weight, float eps);
/* IRS_DATA_MI: the data term of a chain is weight * n * (ln B - MI) (irs_mi_fwd, B = irs_config.lcc_s), alpha[c] = 1, and
 * irs_io.residuals receives mask * (ln B - pmi) (irs_mi_bwd), whose masked sum times weight is the data term.  weight > 0 and the
 * two ranges, finite with hi > lo, travel here because irs_config has no room left; the call is required -- the library does not
 * guess intensity ranges, and a transition of a context that never had it is refused -- and allowed only before the first
 * transition.  Such a context takes no virtual decimation and no z-slab, and its sparse data and sparse forward stages stay off
 * (the sparse adjoint works as ever: the gradient vanishes off the mask). */
int irs_mi_set(irs_ctx* ctx, float weight, float f_lo, float f_hi, float m_lo, float m_hi);
/* IRS_DATA_NGF: the data term of a chain is weight * sum mask * d (irs_ngf_fwd with the mask as u), alpha[c] = 1, and
 * irs_io.residuals receives mask * d.  weight, eps_f and eps_m, finite and > 0, travel here because irs_config has no room left;
 * the call is required -- the library does not guess an edge parameter, and a transition of a context that never had it is
 * refused -- and allowed only before the first transition.  Such a context takes no virtual decimation and no z-slab, and its
 * sparse data and sparse forward stages stay off: the stencil reads beyond the mask (the sparse adjoint works as ever). */
int irs_ngf_set(irs_ctx* ctx, float weight, float eps_f, float eps_m);
/* Switches the context's sampler to SGHMC: the update of a transition becomes the step of irs_sghmc_update on (irs_io.v, momentum)
 * with lr = irs_config.lr, sigma = irs_io.sigma, the context's seed and Philox counter, and grad = grad_v, which irs_io.grad_v
 * still receives; the forward pass adds NO noise -- curr_state is the smoothed v itself -- and irs_io.eps, where given, is the
 * momentum's noise instead.  momentum: the caller's device array (C,3,Dv,Hv,Wv), which must outlive the transitions; a transition
 * that ends as a no-op writes neither v nor momentum, and its re-run draws the same noise.  Jitter, counter, timings, stream
 * capture and every other stage are as without the call.  friction in (0, 1], temperature >= 0 and finite; only before the first
 * transition; not on a z-slab context.  With irs_config.sobolev_s > 0 grad_v is not the gradient of a potential in v (the
 * smoothing's backward is the identity, as in the reference): the chain is then the momentum counterpart of the reference's
 * scheme, textbook SGHMC only with sobolev_s = 0. */
int irs_sghmc_set(irs_ctx* ctx, float friction, float temperature, float* momentum);
/* blocking copies of the small state / scalars.  (A slab context whose transport has failed -- a peer gone, irs_slab_transition /
 * irs_flush return that error -- still answers these two: the device holds the state after the last good transition.) */
int irs_get_state(irs_ctx* ctx, irs_state* out, void* stream);
int irs_set_state(irs_ctx* ctx, const irs_state* in, void* stream);
int irs_get_scalars(irs_ctx* ctx, irs_scalars* out, void* stream);

/* Trainer.__GMM_init (trainer/trainer.py:529-547): init log_std from std(z[mask]) at the given velocity sample
 * (NULL = zero field), then `warm_up` _step_GMM iterations.  blocking (reads one scalar back). */
int irs_gmm_init(irs_ctx* ctx, const irs_io* io, const float* v_sample, int warm_up, void* stream);

/* one SG-MCMC transition.  Asynchronous: nothing is allocated and the DEVICE is never waited for; the host, however, is
 * held back so that it runs at most two transitions ahead of the device (it waits on the end event of the transition before
 * the previous one -- the kernel-variant prediction reads bounds no older than that).  Under stream capture that wait is
 * skipped, so the call stays graph-capturable.  Which variants of the squaring-step kernels get launched is predicted from
 * the displacement bounds of earlier transitions; the device checks the prediction, and a transition that was launched
 * without a variant it turned out to need leaves everything untouched and is re-run by a later call (irs_flush).
 * Consequences for a caller that reads per-call results: the output arrays of irs_io (and grad_v, and the timings of
 * irs_transition_timed) belong to transition t only once irs_flush has returned -- until then a dropped transition leaves them
 * holding an earlier sample.  A re-run draws the in-kernel Philox noise of the transition it repeats (the counter did not
 * advance), but INJECTED eps / unif are taken from the irs_io of the call that performs the re-run: parity runs with injected
 * noise set predict_variants = 0.  Under stream capture no prediction is made and nothing is re-run (the captured sequence
 * launches every variant), so a replayed graph never depends on host state. */
int irs_transition(irs_ctx* ctx, const irs_io* io, void* stream);

/* Wait for everything enqueued on `stream` and complete the chain: a transition whose kernel-variant (or, on a slab, ghost-width)
 * prediction turned out wrong is a NO-OP on the device -- no parameter, optimiser moment, Philox counter or velocity changes --
 * and is re-run without predictions by the next irs_transition / irs_slab_transition call; this call re-runs the ones the last
 * calls left behind (with the irs_io of the most recent call, whose buffers must still be alive).  irs_get_state and
 * irs_get_scalars call it.  After it, v / state / scalars are those of a chain that never mispredicted.  blocking; collective
 * on a slab context (every rank reaches the same verdicts at the same call). */
int irs_flush(irs_ctx* ctx, void* stream);
/* transitions re-run so far because a prediction failed (statistics) */
int irs_recovered_transitions(const irs_ctx* ctx, uint64_t* out);
/* The sparse adjoint of a context on (the default) or off: with 0 the adjoint squaring steps march full columns, the launch sequence
 * as it was before the plan existed -- the same numbers (A/B runs and parity tests).  A call of its own, not a row of irs_option_set:
 * the state lives in the context next to the plan's buffers.  Takes effect with the next transition enqueued. */
int irs_sparse_adjoint_set(irs_ctx* ctx, int on);
/* What the sparse adjoint did in the LAST transition: the adjoint squaring steps march only
 * the planes the gradient of the data term can reach -- per 32 x 8 tile column the z-range around the support of g_warped, widened
 * by one voxel per step, found on the device -- as long as every step of the chain stays below one voxel of displacement.
 * out: int32 [no_steps][no_chains][4] = whether the chain was marched sparsely, the piece length (planes) its columns were cut
 * into, the pieces of the chain in the step's list, the planes in its run ranges (of dims[0] x tile columns).  All zero when
 * switched off, on a slab context, before the first transition, and on a volume so small that the full-column launch already uses
 * the shortest pieces (128^3 with one chain: the lists could only match them).  Calls irs_flush; blocking. */
int irs_sparse_adjoint_get(irs_ctx* ctx, int32_t* out, void* stream);
/* The sparse data stage of a context on (the default) or off.  On: the z-extent of the fixed mask is found on the device in every
 * transition, the warp computes only the 64 x 8 tile-planes within 3 lcc_s voxels of it (SSD: on it), and the LCC map and the data
 * term march piece lists of their 32 x 16 tile columns at reach lcc_s and 2 lcc_s (the data term zero-fills the rest of g_warped;
 * the statistics keep their dense launch).  What is skipped is only ever multiplied by an exact
 * zero: v, grad_v, the state and every scalar equal the dense stage's as numbers, except data_term[c], an fp64 sum whose grouping
 * follows the pieces (it differs by re-association, at most n_masked 2^-52 relative to the sum of |-log p|).  A transition whose
 * irs_io asks for im_moving_warped or residuals runs the dense stage.  on: 0 off; 1 on, where the volume is large enough for lists
 * to be shorter than the full-column segments (see irs_sparse_data_get); n >= 2: on whatever the volume's size, with pieces of at
 * most n planes (at least 4) instead of the shortest that fit one resident set -- for tests and A/B runs on small volumes.  A call
 * of its own, like irs_sparse_adjoint_set. */
int irs_sparse_data_set(irs_ctx* ctx, int on);
/* What the sparse data stage did in the LAST transition.  out: int32 [4][no_chains][4], rows warp, LCC map, statistics, data term;
 * per row and chain: engaged, piece length (planes), entries of the chain in the kernel's list, planes marched -- for the map and
 * the data term planes of 32 x 16 tile columns in run pieces; for the warp, which has no list, tile-planes of 64 x 8 inside the
 * hull (piece length and entries 0); the statistics row is zero (dense launch).  All zero when switched off, on a slab context, before the first
 * transition, when the dense stage ran, and on a volume whose full-column LCC launches already use the shortest pieces (128^3).
 * Calls irs_flush; blocking. */
int irs_sparse_data_get(irs_ctx* ctx, int32_t* out, void* stream);
/* The sparse forward squaring steps of a context on (the default) or off.  On: step k computes d_{k+1} only on the run pieces of
 * its list -- per 64 x 8 tile column the planes within 3 lcc_s + h_{k+1} + ... + h_{n-1} voxels of the fixed mask (SSD: lcc_s = 0),
 * h_i the planned width of step i -- which is where the warp, the steps behind it and the adjoint read it.  The widths are planned on
 * the host from the published bounds max|d_i| (1.25 m + 0.25, as a slab's ghost widths) and checked on the device after the forward
 * pass (floor(max|d_i|) + 1 <= h_i): a transition whose plan does not hold is a no-op that is re-run with dense steps (irs_flush,
 * irs_recovered_transitions).  v, grad_v, the state and every scalar equal the dense steps' as numbers wherever both select the
 * same adjoint variants; the published bounds are maxima over the marched pieces.  Engaged only when the sparse data stage ran in
 * the transition, every width could be planned (a published bound for every step, predict_variants = 1, not a re-run, not a
 * captured stream), no step needs the any-radius adjoint, the context has no FFD and no slab, and the irs_io asks for neither
 * transformation nor displacement (nor im_moving_warped / residuals).  on: 0 off; 1 on, where the dense launch uses segments longer
 * than the shortest piece in its two-rows form (not at 128^3); n >= 2: on whatever the volume's size, with pieces of at most n planes
 * (at least 4) -- for tests and A/B runs.  A call of its own, like irs_sparse_data_set.  Test hook: slab_force_h > 0 (irs_option_set)
 * on a context without a slab forces every planned width to that value. */
int irs_sparse_forward_set(irs_ctx* ctx, int on);
/* What the sparse forward steps did in the LAST transition.  out: int32 [no_steps][no_chains][5] = engaged, piece length (planes),
 * run pieces of the chain in the step's list, planes of 64 x 8 tile columns in its run ranges, planned width of the step.  All zero
 * when the dense steps ran.  Calls irs_flush; blocking. */
int irs_sparse_forward_get(irs_ctx* ctx, int32_t* out, void* stream);
/* How the piece lists of the three sparse stages are kept from transition to transition.  A list is a pure function of its extent
 * table (the fixed mask's, or g_warped's), of the launch shape it is cut for (tile, reach, fill rule, resident set, piece length,
 * chains, dims) and -- the adjoint -- of which chains left the radius-1 kernel; each list keeps a record of those on the device, the
 * extent pass notes whether its table changed, and the launches that would rebuild a list whose record still holds leave at once.
 * Decided on the device, in stream order, from data: a mask that changes under the same pointer is seen in the transition in which
 * it changes, nothing is read back, and the sequence captures into a graph.  reuse: bit 0 (default 1) reuse on, 0 every list is
 * rebuilt in every transition; bit 1 (default 0) the adjoint's lists are always cut from the extents of g_warped -- by default they are
 * cut from the mask's table, at the reach of g_warped's support around the mask more, whenever the sparse data stage formed that
 * table in the transition.  The same numbers either way.  A call of its own, like irs_sparse_data_set. */
int irs_sparse_plan_set(irs_ctx* ctx, int reuse);
/* out: int32 [3][2] = per family (data stage with the warp's hull counted as a list, forward steps, adjoint steps) the lists rebuilt
 * and the lists reused since irs_create, counted on the device.  Calls irs_flush; blocking. */
int irs_sparse_plan_get(irs_ctx* ctx, int32_t* out, void* stream);

/* timing hook for bench.py: the same transition with hipEvents recorded on `stream` around the stages; blocking.
 * All times in milliseconds for THIS call. */
typedef struct irs_timings {
    float total_ms;            /* whole transition */
    float exp_fwd_ms;          /* the no_steps scaling-and-squaring forward launches */
    float exp_bwd_kernel_ms;   /* sum over the no_steps radius-1 adjoint KERNEL launches (events around each launch) */
    float exp_bwd_total_ms;    /* adjoint loop including the gradient-buffer memsets */
    float smooth_ms;           /* perturbation + Sobolev smoothing (+ FFD up-sampling) */
    float data_ms;             /* warp, LCC map, statistics, GMM step, data term + adjoints, warp backward */
    float update_ms;           /* gradient assembly + SGLD update + bookkeeping */
    float exp_bwd_primary_avg_ms; /* mean launch duration of the dominant kernel alone: the radius-1 adjoint step without
                                     input prescale (steps 1 .. no_steps-1), events around exactly that launch -- the
                                     number rocprofv3 reports for exp_bwd_march_kernel<false,1> */
} irs_timings;
int irs_transition_timed(irs_ctx* ctx, const irs_io* io, void* stream, irs_timings* out);

/* ------------------------------------------------------------------------------------------------
 * z-slab decomposition INSIDE the library (BASELINE.json config 4): one chain, the volume split
 * along z over the ranks of a node, one process per GPU.  What is sharded is the single-device loop body
 * trainer/trainer.py:291-356 (the reference has no multi-device code, base/base_trainer.py:16).
 *
 * Rank r owns the planes [a, b) = [r D / n, (r + 1) D / n) and HOLDS [lo, hi) = [a - margin, b + margin) clipped to the
 * volume: every array of the context and every array of irs_io -- except the moving image -- is slab-local,
 * (C, ch, hi - lo, H, W), so memory per rank falls with the number of ranks.  The moving image is static and is given
 * whole (67 MB at 256^3): the warp may then sample it at any displacement without traffic.
 *
 * irs_slab_transition runs the same kernels as irs_transition on windows of the slab and moves ghost planes between
 * neighbouring ranks with the communicator (RCCL ncclSend / ncclRecv groups, or producer-side stores into peer-mapped landing areas, on a
 * communication stream of its own; three small all-reduces per transition -- displacement bounds, statistics per chain, data-term
 * sums together with the regulariser energies) -- no host synchronisation, no Python between the stages:
 *   - stencil halos of fixed width (Sobolev s, LCC 4 s, update 1);
 *   - gather halos of the squaring steps, whose width floor(max|d_k|) + 1 follows the displacement: planned on the host from
 *     the all-reduced bounds of an earlier transition (never waited for), validated on the device afterwards
 *     (irs_slab_status_get); the first transition measures them step by step ("exact" mode, blocking);
 *   - forward squaring steps are grouped into communication-avoiding blocks (one exchange of up to `ghost_max` planes,
 *     then several steps on shrinking windows); every step around an exchange is split into its interior (launched
 *     while the exchange is in flight) and its two boundary strips (launched when the ghost planes have arrived);
 *   - the adjoint is an owner-computes gather, so the backward pass also only RECEIVES ghost planes (of the incoming
 *     gradient): no reverse halo accumulation.
 * With one rank the schedule degenerates to the single-GPU launch sequence.
 * SVFFD_3D: the control grid is small, so v / sigma / eps / curr_state / grad_v stay WHOLE (control-grid sized, replicated on
 * every rank: same Philox noise, same smoothing, same update); the dense velocity is up-sampled on the planes a rank needs,
 * and the adjoint of the up-sampling sums over a rank's own planes, one more all-reduce (floats) making the control-grid
 * gradient whole.
 * ---------------------------------------------------------------------------------------------- */
typedef struct irs_comm irs_comm;
#define IRS_COMM_ID_BYTES 128
/* rank 0: ncclGetUniqueId; the caller distributes the bytes to the other ranks (any channel). */
int irs_comm_unique_id(uint8_t id[IRS_COMM_ID_BYTES]);
/* ncclCommInitRank on the CURRENT device; collective over the `world` ranks, blocking. */
int irs_comm_create_rccl(const uint8_t id[IRS_COMM_ID_BYTES], int rank, int world, irs_comm** out);
/* Peer-mapped transport: every rank exports ONE device allocation (its landing area for ghost planes and all-reduce
 * contributions) with hipIpcGetMemHandle and maps its peers' (hipIpcOpenMemHandle); an exchange is a kernel of the PRODUCER storing
 * its strips into the consumer's landing area (xGMI stores on a node), ordered across processes by sequence flags -- no host or
 * stream synchronisation, no rendezvous.  `name` names a POSIX shared-memory segment through which the handles (and, by default,
 * the flags) travel: the same string on every rank, distributed by the caller like the id above; rank 0 creates the segment and
 * unlinks the name once every rank has attached.  Ranks may share a device (several processes on one GPU: how the asynchronous
 * schedule is exercised on a one-GPU box) or own one each (world <= 8, one node).  Collective, blocking.  Environment:
 * IRS_IPC_SLOT_MB (8) sizes the first landing area (MiB per neighbour and slot; it grows when a context needs more);
 * IRS_IPC_TIMEOUT_S (20) bounds every wait of a kernel for a peer -- a rank that waits longer raises an error that the next
 * irs_slab_transition / irs_flush returns. */
int irs_comm_create_ipc(const char* name, int rank, int world, irs_comm** out);
/* The same two transport operations as caller-supplied functions: rehearsal of the schedule with several ranks sharing ONE
 * GPU, which RCCL refuses (tests).  A callback must leave the data in place when it returns or enqueue its work on `stream`. */
typedef struct irs_xfer {
    void* ptr;      /* device pointer */
    size_t bytes;
    int32_t peer;   /* rank */
    int32_t recv;   /* 0 = send, 1 = receive */
} irs_xfer;
typedef int (*irs_exchange_fn)(void* user, const irs_xfer* xfers, int n, void* stream);
typedef int (*irs_allreduce_fn)(void* user, void* buf, size_t count, int kind, void* stream); /* 0 SUM f64 | 1 MAX u32 | 2 SUM f32 */
int irs_comm_create_callbacks(irs_exchange_fn ex, irs_allreduce_fn ar, void* user, int rank, int world, irs_comm** out);
void irs_comm_destroy(irs_comm* comm);
/* timing hook: `iters` neighbour exchanges of `bytes` (a multiple of 16) per direction and link, then `iters` all-reduces of
 * `ar_doubles` doubles, back to back; usec[0] / usec[1] = host-timed microseconds per exchange / per all-reduce. collective, blocking. */
int irs_comm_probe(irs_comm* comm, size_t bytes, size_t ar_doubles, int iters, void* stream, double usec[2]);
/* one line about the transport (kind, ranks; ipc: size and kind of the landing area, traffic so far) for logs */
int irs_comm_describe(const irs_comm* comm, char* out, size_t n);
int irs_comm_rank(const irs_comm* comm);
int irs_comm_world(const irs_comm* comm);
/* one all-reduce of each kind and one ring exchange on scratch memory, verified on the host. blocking, collective. */
int irs_comm_selftest(irs_comm* comm, void* stream);

typedef struct irs_slab_config {
    int32_t ghost_max;  /* widest ghost zone of one exchange, planes (0 -> 8); lowered to what the thinnest slab can send a
                         * neighbour (slab planes - sobolev_s): irs_slab_layout.ghost_max says what is in force */
    int32_t margin;     /* ghost planes held beyond a neighbour-facing edge (0 -> derived from the stencil widths) */
} irs_slab_config;
typedef struct irs_slab_layout {
    int32_t rank, world;
    int32_t a, b;       /* owned planes */
    int32_t lo, hi;     /* held planes: every slab-local array is (C, ch, hi - lo, H, W) */
    int32_t margin, ghost_max;
} irs_slab_layout;
/* planes a rank would own / hold, without creating anything (pure host arithmetic; what the caller cuts its arrays with) */
int irs_slab_plan_layout(const irs_config* cfg, const irs_slab_config* scfg, int rank, int world, irs_slab_layout* out);
/* context with slab-local workspace; `comm` may be NULL when world == 1.  The communicator is not owned. blocking. */
int irs_slab_create(const irs_config* cfg, const irs_slab_config* scfg, irs_comm* comm, irs_ctx** out);
int irs_slab_get_layout(const irs_ctx* ctx, irs_slab_layout* out);
/* one transition of the slab; irs_io arrays are slab-local except moving_im (whole volume, moving_chains in {1, C}).
 * curr_state / im_moving_warped / residuals outputs are valid on the owned planes.  asynchronous (after the first call). */
int irs_slab_transition(irs_ctx* ctx, const irs_io* io, void* stream);
/* Trainer.__GMM_init on the slabs (v_sample slab-local or NULL); collective, blocking. */
int irs_slab_gmm_init(irs_ctx* ctx, const irs_io* io, const float* v_sample, int warm_up, void* stream);
typedef struct irs_slab_status {
    uint64_t transitions, exact_transitions; /* total / run in exact (measuring, blocking) mode */
    uint64_t exchanges, exchanged_bytes;     /* point-to-point rounds / bytes sent by this rank */
    uint64_t mispredictions;                 /* transitions whose planned ghost widths turned out too narrow (results invalid) */
    int32_t last_fwd_rounds, last_bwd_rounds;/* exchange rounds of the squaring steps in the last transition */
} irs_slab_status;
/* blocking (waits for the enqueued transitions). A non-zero `mispredictions` is also returned as an error by the next
 * irs_slab_transition. */
int irs_slab_status_get(irs_ctx* ctx, irs_slab_status* out, void* stream);
/* Hand-over TIMELINE of one slab transition: what a first run on a node needs in order to tell a slow transport from load imbalance
 * from a serialised interior / boundary split (the reference has no counterpart: base/base_trainer.py:16 is single-device).
 * irs_slab_timeline_arm(ctx, t): the next `t` transitions record timing events around every exchange and all-reduce (a few
 * hipEventRecord per hand-over: off the timed path -- bench.py arms it on its trial transitions); the LAST armed one is kept.
 * irs_slab_timeline_get: blocking; entries in schedule order, *n_entries = how many there were (also when max_entries is smaller),
 * *total_us = first launch .. last launch of that transition on this rank. */
typedef struct irs_slab_timeline_entry {
    int32_t kind;       /* IRS_OP_EXCHANGE | IRS_OP_ALLREDUCE */
    int32_t stage;      /* exchange: the buffer (IRS_SB_*); all-reduce: IRS_AR_* */
    int32_t k, width;   /* exchange: adjoint step that consumes it (-1: none), ghost planes per side */
    float ready_us;     /* since the transition's first launch: the data to hand over was ready on the compute stream (event P) */
    float handover_us;  /* P .. the communication stream finished the hand-over (event R): push, waiting for the peer, drain / reduce */
    float wait_at_us;   /* since the first launch: the compute stream reached the launch that needs R (-1: never waited for) */
    float stall_us;     /* how long the compute stream stood still there (0: the hand-over was hidden behind interior work) */
} irs_slab_timeline_entry;
int irs_slab_timeline_arm(irs_ctx* ctx, int transitions);
int irs_slab_timeline_get(irs_ctx* ctx, irs_slab_timeline_entry* out, int max_entries, int32_t* n_entries, float* total_us, void* stream);

/* The schedule of the squaring steps as pure host arithmetic (tests, documentation): given the per-step ghost widths
 * h[0..n) (= floor(max|d_k|) + 1), the widest exchange and the smallest slab, fill fwd_round[k] / bwd_round[k] with the index
 * of the exchange round step k belongs to, and fwd_width[r] / bwd_width[r] with the planes that round exchanges (round 0 of
 * the forward pass is fed by the widened smoothing stage and exchanges the perturbed velocity instead).  n_buffers: gradient
 * fields the adjoint rotates through -- 2, or 3 as a context of several ranks has (a backward round then spans up to three
 * steps).  Returns the number of rounds through n_fwd / n_bwd; non-zero status if a width exceeds the limits. */
int irs_slab_plan_rounds(const int32_t* h, int n, int ghost_max, int min_slab, int n_buffers, int32_t* fwd_round, int32_t* fwd_width,
                         int32_t* n_fwd, int32_t* bwd_round, int32_t* bwd_width, int32_t* n_bwd);

/* The schedule of one planned transition of rank `rank`, as data -- the list the executor inside irs_slab_transition
 * interprets, built by the same host code (tests replay it on the CPU over two gloo ranks: tests/test_slab_schedule.py).
 * h[0..no_steps): ghost width of every squaring step.  n_ops receives the number of operations (also when max_ops is 0). */
enum { IRS_OP_LAUNCH = 0, IRS_OP_EXCHANGE = 1, IRS_OP_ALLREDUCE = 2, IRS_OP_WAIT = 3 };
enum {  /* launch stages */
    IRS_SG_PERTURB = 0, IRS_SG_COPY_V, IRS_SG_SMOOTH, IRS_SG_ENERGY, IRS_SG_EXP_FWD, IRS_SG_OUTPUTS, IRS_SG_WARP, IRS_SG_RESIDUAL,
    IRS_SG_STATS, IRS_SG_DATA_BWD, IRS_SG_WARP_BWD, IRS_SG_EXP_BWD, IRS_SG_UPDATE, IRS_SG_FFD_UP, IRS_SG_FFD_ADJ,
    IRS_SG_SCALARS = 32,  /* single-workgroup stages from here on (no output window) */
    IRS_SG_CHAIN_SCALAR = 32, IRS_SG_REG_SCALAR, IRS_SG_FINALIZE, IRS_SG_VERDICT
};
enum {  /* buffers */
    IRS_SB_V = 0, IRS_SB_NOISY, IRS_SB_VS, IRS_SB_WARPED, IRS_SB_Z, IRS_SB_GM, IRS_SB_GRAD_A, IRS_SB_GRAD_B,
    IRS_SB_DENSE,      /* SVFFD: the dense velocity (V, NOISY, VS then live on the control grid, replicated on every rank) */
    IRS_SB_GRAD_C,     /* third gradient field of the adjoint (contexts of several ranks) */
    IRS_SB_STEP0 = 16  /* + k: output of squaring step k */
};
enum { IRS_AR_ENERGY = 0, IRS_AR_DMAX = 1, IRS_AR_NLL = 2, IRS_AR_STATS = 3, IRS_AR_CPGRAD = 4, IRS_AR_MOMENTS = 7 };
typedef struct irs_slab_op {
    int32_t kind;              /* IRS_OP_* */
    int32_t stage;             /* launch: IRS_SG_*; exchange: the buffer (IRS_SB_*); all-reduce: IRS_AR_* */
    int32_t k;                 /* squaring step / chain */
    int32_t lo0, hi0, lo1, hi1;/* launch: output window [lo0, hi0) and, for boundary strips, a second one [lo1, hi1) */
    int32_t in0, in1;          /* launch: buffers read with a z reach (-1: none) */
    int32_t reach;             /* launch: planes beyond the output window(s) read from in0 / in1 */
    int32_t out;               /* launch: buffer written (-1: none) */
    int32_t width;             /* exchange: ghost planes per side */
    int32_t id;                /* exchange / all-reduce: its id; wait: the id waited for */
} irs_slab_op;
int irs_slab_trace(const irs_config* cfg, const irs_slab_config* scfg, int rank, int world, const int32_t* h, irs_slab_op* ops,
                   int max_ops, int32_t* n_ops);

/* Tuning / test switches (none of them selects other arithmetic: launch shapes, which always-correct kernel variants get
 * launched, test hooks).  The library reads its IRS_* environment variables ONCE per process, on first use; a context copies
 * them when it is created and no transition calls getenv.  This call changes one switch by name afterwards: on `ctx`, or --
 * ctx == NULL -- process-wide (the stateless operators and every context created later).  Names: predict_variants,
 * run_ahead, fuse_warp_bwd, energy_in_update, fuse_noise, recover, fwd_rows1, coarse_box, sobolev_tile, march_seg,
 * march_seg_fwd, swz_run, seg_min_blocks, seg_min_len, sobolev_seg, lcc_seg, stats_seg, update_seg, slab_split, slab_exact,
 * slab_force_h, slab_buffers, ps_rows, tile_box, data_batch, chain_overlap, launch_log (csrc/common.h: Knobs).  The reference has no counterpart (it has one code path). */
int irs_option_set(irs_ctx* ctx, const char* name, int value);

const char* irs_last_error(void);
const char* irs_version(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* IRSGMCMC_H */
