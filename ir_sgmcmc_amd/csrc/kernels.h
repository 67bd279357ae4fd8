// Host-side launchers of the gfx950 kernels (internal; the public surface is include/irsgmcmc.h).
#pragma once
#include "common.h"
#include "sghmc_device.h"

namespace irs {

struct Taps {
    float k[2 * IRS_MAX_HALF_WIDTH + 1];
    int s;
};

struct SplineTaps {
    float k[32];  // sampled cubic B-spline, 4*cps - 1 taps (cps <= 8)
    int cps;
};

// identity-grid tables live in device memory; built once per (D,H,W)
struct LinTables {
    float* dev = nullptr;  // [W | H | D]
    int D = 0, H = 0, W = 0;
    Lin lin() const { return Lin{dev, dev + W, dev + W + H}; }
};
int ensure_lin_tables(LinTables& t, int D, int H, int W, hipStream_t st);
// process-wide cache used by the stateless operators
int cached_lin(int D, int H, int W, hipStream_t st, Lin* out);

// ---- field_kernels.hip
void launch_perturb(const float* v, const float* sigma, const float* eps, float amp, float* out, int C, Vol vol,
                    uint64_t seed, uint64_t iteration, const uint64_t* dev_iteration, hipStream_t st);
// the SGHMC step (sghmc_device.h) on (v, hm.m) in place, outside a transition: grad is grad_v, every chain in one launch
void launch_sghmc_update(float* v, const float* grad, const float* sigma, float lr, const SghmcArgs& hm, uint64_t iteration, int C, Vol vol,
                         hipStream_t st);
void launch_svf_outputs(const float* d, float* transformation, float* displacement, int C, Vol vol, Lin lin,
                        hipStream_t st);
void launch_warp_fwd(const float* im, int64_t im_stride, const float* d, const float* unif, float alpha, float* out,
                     float* gradm, int gradm_aos, int C, Vol vol, Lin lin, uint64_t seed, uint64_t iteration,
                     const uint64_t* dev_iteration, hipStream_t st, const int* hull = nullptr);  // hull: DataPlan::hull -- tile-planes
                                                                                                 // outside it are left unwritten
void launch_warp_bwd(const float* im, int64_t im_stride, const float* d, const float* unif, float alpha,
                     const float* g_warped, float* g_d, int C, Vol vol, Lin lin, uint64_t seed, uint64_t iteration,
                     const uint64_t* dev_iteration, hipStream_t st);
void launch_warp_transformation(const float* im, int64_t im_stride, const float* t, float* out, int C, Vol vol,
                                hipStream_t st);
void launch_warp_nearest_u8(const uint8_t* im, int64_t im_stride, const float* t, uint8_t* out, int C, Vol vol,
                            hipStream_t st);
void launch_warp_nearest_i16(const int16_t* im, int64_t im_stride, const float* t, int16_t* out, int C, Vol vol,
                             hipStream_t st);
// rows [w_lo, w_lo + w_n) of the dense axis produced (up) / summed (adjoint); the windowed array stores rows
// [store_lo, store_lo + store_n) of that axis.  w_n < 0 / store_n < 0: the whole axis.
void launch_ffd_axis(const float* in, float* out, const SplineTaps& taps, bool adjoint, int64_t outer, int n_in,
                     int n_out, int64_t inner, hipStream_t st, int w_lo = 0, int w_n = -1, int store_lo = 0, int store_n = -1);
void launch_scale_channels(const float* in, float* out, float s0, float s1, float s2, int C, Vol vol, hipStream_t st);

// ---- exp_kernels.hip (z-marching squaring step + owner-computes gather adjoint, LDS-scatter fallback)
// dmax_in: published bound of the input field (nullptr = unknown), dmax_out: receives the bound of the output field
void launch_exp_step_fwd_march(const float* din, float* dout, bool prescale, int no_steps, int C, Vol vol, Lin lin,
                               const unsigned* dmax_in, unsigned* dmax_out, bool only_r1, int lay, hipStream_t st);
// the adjoint is launched as a set: gather radius 1, gather radius 2 and the scatter fallback; exactly one of them does
// the work, chosen on the device from the bound max|d_k|
// plan (adjoint_plan.hip), optional: the radius-1 kernel walks step `step`'s piece list instead of full columns
struct AdjointPlan;
void launch_exp_step_bwd_march(const float* G, const float* dk, float* gout, bool prescale, int no_steps, int C, Vol vol,
                               Lin lin, const unsigned* dmax, int max_radius, bool r2_owns_rest, const float* gscale, int lay,
                               hipEvent_t after_primary, hipStream_t st, const AdjointPlan* plan = nullptr, int step = 0);
int exp_bwd_dense_seg_len(Vol vol, int C);  // z-segment length of the full-column radius-1 launch
int64_t exp_bwd_plan_resident();  // workgroups of the list-walking radius-1 kernel the chip holds at once (0: unknown)
// cmm: scratch of coarse_minmax_bytes(vol, C) for the per-cell displacement extrema (nullptr: sources are bounded by the
// global bound around the tile only -- correct, slow for large displacements)
size_t coarse_minmax_bytes(Vol vol, int C);
void launch_exp_step_bwd_lds(const float* G, const float* dk, float* gout, bool prescale, int no_steps, int C, Vol vol,
                             Lin lin, const unsigned* dmax, int halo, int gather_radius, const float* gscale, int lay,
                             float* cmm, hipStream_t st);
void launch_field_absmax(const float* d, bool prescale, int no_steps, unsigned* dmax, int C, Vol vol, hipStream_t st);

// ---- adjoint_plan.hip (which planes the adjoint squaring steps march: the support of the incoming gradient, on the device)
struct PlanEntry;
struct ColPlan;
struct PlanRecord;
struct DataPlan;
struct AdjointPlan {   // views into one allocation of adjoint_plan_bytes()
    int* ext = nullptr;            // [C][H W][2]: (D - lo, hi) of the planes where g_warped != 0, per voxel column
    int* runs = nullptr;           // [no_steps][C tiles][2]: run range of every tile column
    ColPlan* colplan = nullptr;    // [no_steps][C tiles]: run range + fills of every tile column (scratch of the list kernel)
    PlanEntry* entries = nullptr;  // [no_steps][cap]
    int* count = nullptr;          // [no_steps][2] entries of a step's list, and how many of them (the first) are run pieces
    int* stats = nullptr;          // [no_steps][C][kPlanStats]
    PlanRecord* rec = nullptr;     // [no_steps]: what every list was cut from (adjoint_plan.h: plan reuse)
    unsigned long long* gen = nullptr;  // generation of `ext`
    int* counters = nullptr;       // {lists rebuilt, lists reused} since irs_create
    int cap = 0, ntx = 0, nty = 0;
};
size_t adjoint_plan_bytes(Vol vol, int C, int no_steps);
AdjointPlan adjoint_plan_views(char* base, Vol vol, int C, int no_steps);
// extents of g_warped ([C][V]) -> run ranges -> piece lists of all steps; dmax: [no_steps][C][4] bounds of d_k; G: resident set
// the lists are cut for; forced_len > 0: that piece length.  mask_table: the data plan whose extent table of the MASK this transition
// has formed (mask_chains chains; S: LCC half width, SSD 0) -- the lists are cut from it at reach 2 S + (n - k), a superset of the
// gradient's support, and g_warped is not scanned; nullptr: from g_warped's own extents.  reuse bit 0: lists whose record holds stay
void launch_adjoint_plan(const float* g_warped, const DataPlan* mask_table, int mask_chains, int S, const unsigned* dmax, const AdjointPlan& plan,
                         int no_steps, int C, Vol vol, int64_t G, int forced_len, int reuse, hipStream_t st);
// Sparse forward steps: one run-piece list per squaring step over the 64 x 8 columns of the forward tile, from the extent table of
// the data plan (`ext`, formed in front of the forward pass) and the widths the host planned: list k (the step that writes d_{k+1})
// is the hull of mask (+) (3 S + width[k+1] + ... + width[n-1]).  The views are an AdjointPlan without an extent table of its own.
size_t forward_plan_bytes(Vol vol, int C, int no_steps);
AdjointPlan forward_plan_views(char* base, Vol vol, int C, int no_steps);
int forward_plan_run_bound(const AdjointPlan& plan, int C, Vol vol, int64_t G, int forced_len);  // most run pieces a step's list can have
// the forward step on step `step`'s list (exp_kernels.hip): the radius-1 tile body, bound of the marched pieces into dmax_out
void launch_exp_step_fwd_plan(const float* din, float* dout, bool prescale, int no_steps, int C, Vol vol, Lin lin, unsigned* dmax_out, int lay,
                              const AdjointPlan& plan, int step, int forced_len, hipStream_t st);
int64_t exp_fwd_plan_resident();  // workgroups of the list-walking forward kernel the chip holds at once (0: unknown)
// the rule on sizes of the sparse forward steps: the dense launch uses segments longer than the shortest piece, and not its small form
bool exp_fwd_dense_allows_lists(Vol vol, int C);
// Sparse data stage: the z-extent of the fixed mask per voxel column -> the warp's hull and the piece lists of the
// data term (list 0) and the LCC map (list 1).  Views into one allocation of data_plan_bytes().
struct DataPlan {
    int* ext = nullptr;            // [mask chains][H W][2]: (D - lo, hi) of the planes where mask != 0
    int* runs = nullptr;           // [2][C tiles][2]: run ranges of the 32 x 16 tile columns at reach 2 s (data term) and s (map)
    int* hull = nullptr;           // [C][64 x 8 tiles][2]: planes of a tile column within 3 s (SSD: 0) of the mask
    ColPlan* colplan = nullptr;    // [2][C tiles]
    PlanEntry* entries = nullptr;  // [2][cap]
    int* count = nullptr;          // [2][2] entries of a list, and how many of them (the first) are run pieces
    int* stats = nullptr;          // [2][C][kPlanStats]
    double* nll = nullptr;         // [cap]: -log p summed over run piece i of the data term's list
    PlanRecord* rec = nullptr;     // [3]: the two lists and the hull (adjoint_plan.h: plan reuse)
    unsigned long long* gen = nullptr;  // generation of `ext`
    int* counters = nullptr;       // {lists rebuilt, lists reused} since irs_create (the hull counts as a list)
    int cap = 0, ntx = 0, nty = 0, wtx = 0, wty = 0;
    int forced_len = 0;            // > 0: the piece length of both lists (irs_sparse_data_set); 0: the shortest that fits a resident set
};
size_t data_plan_bytes(Vol vol, int C);
DataPlan data_plan_views(char* base, Vol vol, int C);
// mask: (mask_chains, V), mask_chains 1 or C; s: LCC half width (0: SSD); lists: false builds the hull alone.  The lists are cut for
// the resident sets of the list-walking LCC kernels, or to plan.forced_len.  fplan (optional): the forward steps' lists in the same
// launches, from the planned widths `width` (list k: the hull of mask (+) (3 S + width[k+1] + ... + width[n-1])).  reuse as above
void launch_front_plans(const uint8_t* mask, int mask_chains, const DataPlan& plan, int s, bool lists, const AdjointPlan* fplan, const int* width,
                        int no_steps, int64_t fwd_G, int fwd_forced, int C, Vol vol, int reuse, hipStream_t st);
// most run pieces the data term's (bwd) / the map's list can have: the marching grid of its kernel
int data_plan_run_bound(const DataPlan& plan, int s, bool bwd, int C, Vol vol);

// ---- data_kernels.hip
void launch_sobolev_march(const float* in, float* out, const Taps& taps, int planes, Vol vol, unsigned* dmax0, int no_steps,
                          hipStream_t st);  // z-marching version (stencil_kernels.hip)
// SGLD perturbation generated while the smoothing kernel stages its planes (SVF_3D path, s > 0): v + noise is never materialised
void launch_perturb_sobolev_march(const float* v, const float* sigma, const float* eps, float amp, float* out, const Taps& taps,
                                  int C, Vol vol, unsigned* dmax0, int no_steps, uint64_t seed, uint64_t iteration,
                                  const uint64_t* dev_iteration, hipStream_t st);  // stencil_kernels.hip
void launch_lcc_fwd_march(const float* fhat, int64_t fhat_stride, const float* im, float* z, float* sigma_out, int s, int C,
                    Vol vol, hipStream_t st);  // z-marching version (stencil_kernels.hip)
// the same tile body walking the run pieces of the map's list (DataPlan, list 1): z, sigma_out outside the pieces stay as they were
void launch_lcc_fwd_plan(const float* fhat, int64_t fhat_stride, const float* im, float* z, float* sigma_out, int s, int C, Vol vol,
                         const DataPlan& plan, hipStream_t st);
int64_t lcc_plan_resident(int s, bool bwd, bool batch);  // workgroups of a list-walking LCC kernel the chip holds at once (0: unknown)
int lcc_dense_seg_len(Vol vol, int C, bool bwd);         // z-segment length of the full-column LCC launches
struct GmmDev;  // device-side mixture parameters (scalar_kernels.hip)
// data term + its gradient w.r.t. the warped image (LCC adjoint fused); mode: IRS_DATA_*.  C_launch > 1 (GMM / LCC only): that many
// chains from `chain` on in one launch -- z, sigma_m, g_warped and the partial sums at their chain offsets, fhat / mask every
// f_stride / mask_stride elements, the mixture of each chain from its snapshot (scalar_kernels.h: DevState::snapA)
void launch_data_bwd(int mode, const float* fhat_or_fixed, int64_t f_stride, const float* z, const float* sigma_m,
                     const uint8_t* mask, int64_t mask_stride, const float* g_z_override, const void* dev_state,
                     int chain, float* g_warped, double* nll_partials, int s, int C_launch, Vol vol, hipStream_t st, int seg_C = 1);
// K: number of mixture components if the caller knows it (selects the K <= 4 build of the kernel), 0 = unknown
void launch_stats(int want_vd, const float* z, const uint8_t* mask, const void* dev_state, double* partials, Vol vol,
                  hipStream_t st, int K = 0);
void launch_residual_ssd(const float* fixed, int64_t f_stride, const float* warped, float* z, int C, Vol vol,
                         hipStream_t st);
// z-marching fused data-term backward (stencil_kernels.hip)
// seg_C: chains the segment length is chosen for (1: a launch per chain; C: all chains in one launch -- longer segments, one resident set)
int lcc_data_bwd_march_blocks(Vol vol, int seg_C = 1);
void launch_lcc_data_bwd_march(const float* fhat, const float* z, const float* sigma_m, const uint8_t* mask,
                               const float* g_z_override, const void* dev_state, int chain, float* g_warped,
                               double* nll_partials, int s, Vol vol, hipStream_t st, int batch = 0, int64_t f_stride = 0,
                               int64_t m_stride = 0, int seg_C = 1);  // batch > 0: chains chain .. chain + batch - 1 in one launch, each against its snapshot
// the same tile body walking the data term's list (DataPlan, list 0): run pieces marched, the rest of g_warped zero-filled, -log p
// per run piece into plan.nll.  C == 1: the mixture in force; C > 1: every chain against its snapshot, as `batch` above
void launch_lcc_data_bwd_plan(const float* fhat, int64_t f_stride, const float* z, const float* sigma_m, const uint8_t* mask,
                              int64_t m_stride, const void* dev_state, float* g_warped, int s, int C, Vol vol, const DataPlan& plan,
                              hipStream_t st);
int data_bwd_blocks(int mode, Vol vol, int seg_C = 1);
void launch_masked_moments(const float* z, const uint8_t* mask, double* partials, Vol vol, hipStream_t st);
void launch_reg_energy(const float* v, double* partials, int C, Vol vol, hipStream_t st);
void launch_reduce_partials(const double* partials, int nblocks, int nvals, double* out, hipStream_t st);
// out[j] = sum_b partials[b * ncols + j]
void launch_reduce_cols(const double* partials, int nblocks, int ncols, double* out, hipStream_t st);
// energy_partials (optional, [C][sgld_update_blocks_per_chain]): regulariser energy of v_s as a by-product; coef_from_w: the
// regulariser coefficient is w / 2 from the state (L2 family) instead of the one reg_scalar_kernel left in the state
// hm (optional): the SGHMC step on (v, hm->m) in place of v <- v - lr grad_v (sghmc_device.h)
void launch_sgld_update(float* v, const float* sigma, const float* g_d0, const float* v_s, const void* dev_state,
                        float lr, float s0, float s1, float s2, float* grad_out, int C, Vol vol, hipStream_t st,
                        double* energy_partials = nullptr, bool coef_from_w = false, const SghmcArgs* hm = nullptr);
int sgld_update_blocks_per_chain(Vol vol, int C);
void launch_gradient_operator(const float* v, float* nabla, int transformation, int C, Vol vol, hipStream_t st);
void launch_log_det_jacobian(const float* t, float* log_det, long long* nan_count, int C, Vol vol, hipStream_t st);
void launch_stats_march(int want_vd, const float* z, const uint8_t* mask, const void* dev_state, double* partials, int blocks,
                        Vol vol, int K, hipStream_t st);  // stencil_kernels.hip
void launch_reg_energy_march(const float* v, double* partials, int blocks, int C, Vol vol, hipStream_t st);
void launch_sgld_update_march(float* v, const float* sigma, const float* g_d0, const float* v_s, const void* dev_state,
                              float lr, float s0, float s1, float s2, float* grad_out, int C, Vol vol, hipStream_t st,
                              double* energy_partials = nullptr, bool coef_from_w = false, const SghmcArgs* hm = nullptr);
int stats_blocks(Vol vol);
int energy_blocks(Vol vol);

// ---- bending_kernels.hip: the second-order operator (HessianOperator) -- energy, gradient and the fused update
// partials: [C][blocks] doubles (blocks = energy_blocks(vol), as for launch_reg_energy)
void launch_bending_energy(const float* v, double* partials, int blocks, int C, Vol vol, hipStream_t st);
// out = scale_c * 2 H^T W H v; scale: C floats on the device or nullptr (= 1)
void launch_bending_grad(const float* v, const float* scale, float* out, int C, Vol vol, hipStream_t st);
// launch_sgld_update with the bending stencil; the coefficient is always the one the scalar stage left in the state
void launch_sgld_update_bending(float* v, const float* sigma, const float* g_d0, const float* v_s, const void* dev_state, float lr,
                                float s0, float s1, float s2, float* grad_out, int C, Vol vol, hipStream_t st,
                                const SghmcArgs* hm = nullptr);

// ---- metric_kernels.hip: average surface distance of label contours (utils/util.py:152-206)
struct SurfLabels {
    int32_t v[IRS_MAX_LABELS];
};
// one (chain, label) pair: its box [z0, z0 + nz) x [y0, y0 + ny) x [x0, x0 + nx), where its voxels start in the box arrays,
// and its first task in each pass.  The table has n_pairs + 1 entries; the last one holds the totals.
struct SurfPair {
    int32_t z0, y0, x0, nz, ny, nx;
    int64_t vox;
    int64_t tw, th, td;
};
constexpr int kSurfLdsLine = 64;  // longest line whose lower envelope stays in LDS (64 entries x 64 lanes x 12 B = 48 KB)
void launch_surface_boxes(const int16_t* fixed, int64_t f_stride, const int16_t* moving, const SurfLabels& lab, int L,
                          int32_t* boxes, int C, Vol vol, hipStream_t st);
// pass W (contours + 1-D distances), passes H and D (lower envelopes; D ends in the reduction) and the per-pair reduction.
// env_scratch: NULL -> the envelopes of a pass live in LDS (its longest line <= kSurfLdsLine); else env_slots slots of
// 3 * line * lanes floats each.  counts == NULL: the passes alone, without the per-pair reduction (surface_kernels.hip reads
// the squared distances pass D kept).
struct SurfPassArgs {
    const SurfPair* plan;
    int P;
    int64_t tasks[3];     // W, H, D
    int line[3];          // longest line of passes H and D (index 1, 2)
    int lanes;            // lanes of an envelope slot in global memory (<= 64)
    float* env_scratch[3];
    int env_slots[3];
    uint8_t* memb;
    float* gA;
    float* gB;
    double* partials;     // 4 per task of pass D: nA, nB, sum A->B, sum B->A
    uint32_t* maxpart;    // NULL: the ASD alone.  Else pass D keeps the squared distances in gA / gB and writes 2 per task: the
                          // largest d2 (float bits) over A of the distance to B, over B of the distance to A
};
void launch_surface_distance(const int16_t* fixed, int64_t f_stride, const int16_t* moving, const SurfLabels& lab, int L,
                             const float spacing[3], const SurfPassArgs& a, long long* counts, double* sums, Vol vol,
                             hipStream_t st);

// ---- hausdorff_kernels.hip: exact order statistics of the contour distances that pass D kept (maxpart != NULL above)
// Direction 0 = the distances of the voxels of A to B (membership bit 1, values in gB), direction 1 = of B to A (bit 2, gA).
// MSB-first radix select on the float bits, 8 bits per pass: per pass one histogram launch (blocks = slices x 2P, integer
// counts in LDS, then integer global atomics) and one scan launch that narrows every rank to its bin.
struct HdArgs {
    const SurfPair* plan;
    int P, Q, slices;
    double pct[IRS_HAUSDORFF_MAX_PERCENTILES];
    const uint8_t* memb;
    const float* gA;
    const float* gB;
    const long long* counts;  // (P,2) of the reduction: |A|, |B|
    const uint32_t* maxpart;
    uint32_t* hist;           // [4 passes][2P][Q][256], zero on entry
    uint32_t* prefix;         // [2P][Q]: the key bits fixed so far
    long long* rank;          // [2P][Q]: 0-based rank among the keys that share the prefix; -1: an empty contour
    double* hd;               // (P,2)
    double* hd_pct;           // (Q,P,2)
};
void launch_hausdorff_select(const HdArgs& a, hipStream_t st);

// ---- surface_kernels.hip: surface posterior (absent in the reference): per fixed-contour voxel the Welford moments of the signed
// distance to every chain's moving contour of the same label, from the squared distances pass D kept (maxpart != NULL above)
// fixed (V) int16 shared by the chains, moving (C,V) int16; plan / gB: of the passes just run on the same maps with the pairs
// c * L + l; mean / m2 (V) float32, count (V) int32, touched at the fixed-contour voxels of the listed labels only
void launch_surface_posterior_update(const int16_t* fixed, const int16_t* moving, const SurfLabels& lab, int L, const SurfPair* plan,
                                     const float* gB, int C, float* mean, float* m2, int32_t* count, Vol vol, hipStream_t st);
struct SurfLevels {
    double z[IRS_SURFACE_MAX_LEVELS];
    int n;
};
// bias / std (V) float32; isummary (L, IRS_SURFACE_SUMMARY_INTS) int64, fsummary (L, IRS_SURFACE_SUMMARY_FLOATS) doubles;
// ws: IRS_SURFACE_WS_BYTES (per label the partials of at most IRS_SURFACE_MAX_BLOCKS blocks)
void launch_surface_posterior_finalize(const int16_t* fixed, const SurfLabels& lab, int L, const float* mean, const float* m2,
                                       const int32_t* count, const uint8_t* mask, const SurfLevels& lv, float* bias, float* std,
                                       long long* isummary, double* fsummary, void* ws, Vol vol, hipStream_t st);

// ---- diag_kernels.hip: split-R-hat and split ESS over chains (absent in the reference; BDA3 sections 11.4-11.5)
// Welford update of one half's (mean, m2) with the sample x, all flat arrays of n floats; k = samples in the half after this one
void launch_chain_moments(const float* x, float* mean, float* m2, int64_t n, int k, hipStream_t st);
// mean / m2: (2,C,3,V); rhat: V floats; summary: 5 doubles {voxels, above thr0, above thr1, max, sum};
// partials: 5 * split_rhat_blocks(V) doubles
int split_rhat_blocks(int64_t V);
void launch_split_rhat(const float* mean, const float* m2, int C, int n, const uint8_t* mask, float thr0, float thr1, float* rhat,
                       double* summary, double* partials, int64_t V, hipStream_t st);
// split ESS (BDA3 section 11.5).  x (C,E), ring (L,C,E), vsum (L,E) with E = 3V; k = position in the current half after x:
// vsum[t-1] += sum over chains of (x - ring[(k-1-t) mod L])^2 for t = 1 .. min(k-1, L), then ring[(k-1) mod L] = x
void launch_chain_variogram(const float* x, float* ring, float* vsum, int C, int64_t E, int L, int k, hipStream_t st);
// ess / mcse: V floats; summary: 5 doubles {voxels, ESS below thr, truncated, min ESS, sum of ESS};
// partials: 5 * split_rhat_blocks(V) doubles
void launch_split_ess(const float* mean, const float* m2, const float* vsum, int C, int n, int L, const uint8_t* mask, float thr,
                      float* ess, float* mcse, double* summary, double* partials, int64_t V, hipStream_t st);

// ---- label_kernels.hip: posterior label maps of the propagated segmentation (absent in the reference)
// seg (C,V) int16; counts (K,V) int32, += 1 per record; volume (K,2) double {mean, M2} of the per-record volumes, folded with
// k = records_before + c + 1; partials: C * K int32 per block of the update (label_update_partials_blocks(V) blocks at most)
int label_update_partials_blocks(int64_t V);
void launch_label_update(const int16_t* seg, int C, int64_t V, const SurfLabels& lab, int K, int32_t* counts, double* volume,
                         int records_before, int32_t* partials, hipStream_t st);
// the second half of the update alone: nblocks rows of C * K int32 block partials summed in block order, then folded into volume
void launch_label_volume_fold(const int32_t* partials, int nblocks, int C, int K, double* volume, int records_before, hipStream_t st);
// entropy (V) float32, map_label (V) int16, summary (K, 6 + 3 * IRS_LABEL_BINS) int64, mask_summary 4 doubles;
// partials: K * (6 + 3 * IRS_LABEL_BINS) int64 and dpartials: 4 doubles per block (label_finalize_blocks(V) blocks)
int label_finalize_blocks(int64_t V);
void launch_label_finalize(const int32_t* counts, int K, int64_t V, int n, const SurfLabels& lab, const int16_t* seg_fixed,
                           const uint8_t* mask, float* entropy, int16_t* map_label, long long* summary, double* mask_summary,
                           long long* partials, double* dpartials, hipStream_t st);

// ---- jacobian_kernels.hip: Jacobian posterior maps (absent in the reference); det J from jacobian_device.h
// t (C,3,V) float32; folds (V) int32, mean / m2 (V) float32: fold count and Welford moments of log det J over the valid records,
// the C chains folded in order after `records_before` records
void launch_jacobian_update(const float* t, int C, int32_t* folds, float* mean, float* m2, int records_before, Vol vol,
                            hipStream_t st);
// fold_prob / logj_mean / logj_std (V) float32; isummary IRS_JACOBIAN_SUMMARY_INTS int64, fsummary IRS_JACOBIAN_SUMMARY_FLOATS
// doubles; ws: IRS_JACOBIAN_WS_BYTES (the per-block partials of at most 1024 blocks: summary_device.h)
void launch_jacobian_finalize(const int32_t* folds, const float* mean, const float* m2, int64_t V, int n, const uint8_t* mask,
                              float* fold_prob, float* logj_mean, float* logj_std, long long* isummary, double* fsummary,
                              void* ws, hipStream_t st);

// ---- structure_kernels.hip: structure report (absent in the reference); arithmetic in structure_device.h
// blocks per row of both first stages, and the bytes of partials `rows` rows (chains, or maps) of K structures need
int structure_blocks(int64_t V);
size_t structure_workspace_bytes(int64_t V, int K, int64_t rows);
// displacement, transformation (C,3,V) float32; seg_fixed (V) int16 shared by the chains; mask (V) uint8 or nullptr; scale: 3 host
// floats; ints (C,K,IRS_STRUCTURE_MOTION_INTS) int64, floats (C,K,IRS_STRUCTURE_MOTION_FLOATS) doubles; ws: structure_workspace_bytes
void launch_structure_motion(const float* displacement, const float* transformation, const int16_t* seg_fixed, const SurfLabels& lab,
                             int K, const uint8_t* mask, const float* scale, long long* ints, double* floats, void* ws, int C, Vol vol,
                             hipStream_t st);
// maps (M,V) float32, any M >= 1; ints (M,K,IRS_STRUCTURE_MAP_INTS) int64, floats (M,K,IRS_STRUCTURE_MAP_FLOATS) doubles
void launch_structure_map_stats(const float* maps, int64_t M, int64_t V, const int16_t* seg_fixed, const SurfLabels& lab, int K,
                                const uint8_t* mask, long long* ints, double* floats, void* ws, hipStream_t st);

// ---- truth_kernels.hip: known-transformation validation (absent in the reference); arithmetic in truth_device.h
// displacement (C,3,V), truth (3,V) float32; below (3,V) uint16; mask (V) uint8 or nullptr; scale: 3 host floats; ints (C,
// IRS_TRUTH_UPDATE_INTS) int64, floats (C,IRS_TRUTH_UPDATE_FLOATS) doubles; ws: IRS_TRUTH_UPDATE_WS_BYTES
void launch_truth_update(const float* displacement, int C, const float* truth, uint16_t* below, const uint8_t* mask, const float* scale,
                         int records_before, int64_t V, long long* ints, double* floats, void* ws, hipStream_t st);
// mean (3,V), comoment (6,V) after n records; d2_edges (B - 1), levels (L), var_edges (R - 1): host doubles; counts
// (IRS_TRUTH_COUNTS(B, L, Br)) int64; rel_ints (R), rel_floats (R,2); ws: IRS_TRUTH_CALIBRATE_WS_BYTES
void launch_truth_calibrate(const float* mean, const float* comoment, const uint16_t* below, const float* truth, int64_t V, int n,
                            const float* scale, double std_floor, const uint8_t* mask, const double* d2_edges, int B,
                            const double* levels, int L, int Br, const double* var_edges, int R, float* error, float* mahalanobis,
                            long long* counts, long long* rel_ints, double* rel_floats, long long* isummary, double* fsummary,
                            void* ws, hipStream_t st);

// ---- covariance_kernels.hip: displacement covariance posterior (absent in the reference); arithmetic in covariance_device.h
// x (C,3,V) float32; mean (3,V), comoment (6,V: xx, yy, zz, xy, xz, yz) float32: Welford moments, the C chains folded in order
// after `records_before` records
void launch_covariance_update(const float* x, int C, float* mean, float* comoment, int records_before, Vol vol, hipStream_t st);
// stdev / direction (3,V), anisotropy (V) float32; scale: 3 host floats; isummary IRS_COVARIANCE_SUMMARY_INTS int64, fsummary
// IRS_COVARIANCE_SUMMARY_FLOATS doubles; ws: IRS_COVARIANCE_WS_BYTES (the partials of at most 1024 blocks)
void launch_covariance_finalize(const float* mean, const float* comoment, int64_t V, int n, const float* scale, const uint8_t* mask,
                                float* stdev, float* direction, float* anisotropy, long long* isummary, double* fsummary, void* ws,
                                hipStream_t st);

// ---- image_posterior_kernels.hip: volumes carried through every recorded transformation (absent in the reference)
// volumes (S,V), t (C,3,V) float32; mean, m2, low, high (S,V) float32: the C samples of every volume folded in chain order after
// `records_before` records (0 overwrites the state); the sample is launch_warp_transformation's, bit for bit.  The grid is
// (ceil(W / 64), ceil(H / 4), D * ceil(S / kImagePosteriorGroup)): a thread owns one voxel of a group of volumes
constexpr int kImagePosteriorGroup = 2;
void launch_image_posterior_update(const float* volumes, int S, const float* t, int C, float* mean, float* m2, float* low,
                                   float* high, int records_before, Vol vol, hipStream_t st);
// one volume's state (V) after n records, reference (V) or nullptr -> std_out, range_out, z_out (V; nullptr with the reference);
// isummary IRS_IMAGE_POSTERIOR_SUMMARY_INTS int64, fsummary IRS_IMAGE_POSTERIOR_SUMMARY_FLOATS doubles; ws:
// IRS_IMAGE_POSTERIOR_WS_BYTES (the partials of at most 1024 blocks)
void launch_image_posterior_finalize(const float* mean, const float* m2, const float* low, const float* high, int64_t V, int n,
                                     const float* reference, float std_floor, const uint8_t* mask, float* std_out, float* range_out,
                                     float* z_out, long long* isummary, double* fsummary, void* ws, hipStream_t st);

// ---- compare_kernels.hip: posterior comparison (absent in the reference); arithmetic in compare_device.h
// mean_x (3,V), comoment_x (6,V) float32 after n_x >= 2 records; scale: 3 host floats; shift, log_std_ratio, bures, jeffreys (V)
// float32; isummary IRS_COMPARE_SUMMARY_INTS int64, fsummary IRS_COMPARE_SUMMARY_FLOATS doubles; ws: IRS_COMPARE_WS_BYTES (the
// partials of at most 1024 blocks)
void launch_posterior_compare(const float* mean_a, const float* comoment_a, int n_a, const float* mean_b, const float* comoment_b,
                              int n_b, int64_t V, const float* scale, double std_floor, const uint8_t* mask, float* shift,
                              float* log_std_ratio, float* bures, float* jeffreys, long long* isummary, double* fsummary, void* ws,
                              hipStream_t st);

// ---- quantile_kernels.hip: displacement credible intervals (absent in the reference); arithmetic in quantile_device.h
// x (C,3,V) float32; centre (3,V) float32, hist (3,bins,V) uint16: the C chains counted after `records_before` records
// (0: centre = chain 0 and hist overwritten); inv_width: 3 host floats
void launch_quantile_update(const float* x, int C, float* centre, uint16_t* hist, int bins, const float* inv_width,
                            int records_before, Vol vol, hipStream_t st);
// quantiles (P,3,V), ci_width (V) float32; width, scale: 3 host floats each; probs: P host doubles; isummary
// IRS_QUANTILE_SUMMARY_INTS int64, fsummary IRS_QUANTILE_SUMMARY_FLOATS doubles; ws: IRS_QUANTILE_WS_BYTES (the partials of
// at most 1024 blocks)
void launch_quantile_finalize(const float* centre, const uint16_t* hist, int bins, int64_t V, int n, const float* width,
                              const float* scale, const double* probs, int P, const uint8_t* mask, float* quantiles,
                              float* ci_width, long long* isummary, double* fsummary, void* ws, hipStream_t st);

// ---- inverse_kernels.hip: inverse transformation and inverse-consistency error (absent in the reference)
void launch_negate(const float* in, float* out, int64_t n, hipStream_t st);
// t_a, d_a, d_b (C,3,V) float32; scale: 3 host floats; mask (mask_chains,V) uint8 or nullptr; residual (C,3,V) / norm (C,V) or
// nullptr; isummary (C, IRS_ICE_SUMMARY_INTS) int64, fsummary (C, IRS_ICE_SUMMARY_FLOATS) doubles; ws: IRS_ICE_WS_BYTES (per
// chain the partials of at most 1024 blocks)
void launch_inverse_consistency(const float* t_a, const float* d_a, const float* d_b, const float* scale, const uint8_t* mask,
                                int mask_chains, float* residual, float* norm, long long* isummary, double* fsummary, void* ws,
                                int C, Vol vol, hipStream_t st);
// norm (C,V) float32 -> mean / peak (V) float32: Welford mean and running maximum of the finite values, the C chains folded in
// order after `records_before` records
void launch_inverse_consistency_update(const float* norm, int C, int64_t V, float* mean, float* peak, int records_before,
                                       hipStream_t st);
// isummary IRS_ICE_MAP_SUMMARY_INTS int64, fsummary IRS_ICE_MAP_SUMMARY_FLOATS doubles; ws: IRS_ICE_MAP_WS_BYTES
void launch_inverse_consistency_finalize(const float* mean, const float* peak, int64_t V, const uint8_t* mask, float threshold,
                                         long long* isummary, double* fsummary, void* ws, hipStream_t st);

// ---- native_kernels.hip: the transformation applied on the image's own voxel grid (absent in the reference)
// Axis order (D, H, W) in every array of three but out_scale, which is per channel (channel c belongs to axis 2 - c).
struct NativeGeom {
    int n[3], p[3], P[3], m[3];  // native shape, padding per side, padded extent n + 2 p, registration grid
    float grid_step[3];          // (m - 1) / (P - 1): grid voxels per padded native voxel
    float half_extent[3];        // (P - 1) / 2: padded native voxels per unit of normalised displacement
    float out_scale[3];          // factor of the displacement output
    float fill;                  // what the pad of the image holds
};
// u (C,3,m) float32; im float32 / seg int16 / mask uint8: (1 or C, n) with moving_stride 0 or n0 n1 n2, or nullptr; the
// outputs (C,n) and disp_out (C,3,n), or nullptr; a volume must be given for every output asked for, at least one output
void launch_native_warp(const float* u, const float* im, const int16_t* seg, const uint8_t* mask, int64_t moving_stride,
                        float* im_out, int16_t* seg_out, uint8_t* mask_out, float* disp_out, const NativeGeom& gm, int C,
                        hipStream_t st);

// ---- native_posterior_kernels.hip: the label and image posteriors on the image's own voxel grid (absent in the reference)
// u (C,3,m) float32; im float32 / seg int16: (1 or C, n) with moving_stride 0 or n0 n1 n2.  seg, counts (K,n) int32, volume (K,2)
// double and partials (C * K int32 per block, native_posterior_blocks(gm) blocks) go together or are all nullptr; so do im and
// mean / m2 / low / high (n) float32; at least one of the two groups.  The C samples are folded in chain order after
// `records_before` records (0 overwrites the image state); gm.fill is what the pad of the image holds
int native_posterior_blocks(const NativeGeom& gm);
void launch_native_posterior_update(const float* u, const float* im, const int16_t* seg, int64_t moving_stride, const SurfLabels& lab,
                                    int K, int32_t* counts, double* volume, int32_t* partials, float* mean, float* m2, float* low,
                                    float* high, int records_before, const NativeGeom& gm, int C, hipStream_t st);

// ---- similarity_kernels.hip: joint intensity histogram, MI / NMI, MSE and NCC of two images (absent in the reference)
struct SimBins {
    int bins;
    float f_lo, f_hi, f_inv;  // range of the fixed image and bins / (hi - lo), formed in fp32
    float m_lo, m_hi, m_inv;  // of the moving image
};
// fixed (1 or C,V) with fixed_stride 0 or V; moving (C,V); mask (V) uint8 or nullptr; hist (C,bins,bins) int32 (zeroed on the
// stream here); stats (C, IRS_SIMILARITY_STATS); ipart / fpart: IRS_SIMILARITY_MAX_BLOCKS rows of 3 int64 / 6 doubles
void launch_image_similarity(const float* fixed, int64_t fixed_stride, const float* moving, const uint8_t* mask, int64_t V, int C,
                             const SimBins& bn, int32_t* hist, double* stats, long long* ipart, double* fpart, hipStream_t st);

// ---- landmark_kernels.hip: a displacement sampled at K points, and the posterior of the mapped landmarks (absent in the reference)
// points, offset (K,3) float32 (offset may be nullptr); displacement (C,3,V); scale: 3 host floats; sampled / mapped (C,K,3)
// float32, either may be nullptr
void launch_transform_points(const float* points, int K, const float* displacement, const float* scale, const float* offset,
                             float* sampled, float* mapped, int C, Vol vol, hipStream_t st);
// mapped (C,K,3), target (K,3) float32; mean (K,3), comoment (K,6: xx, xy, xz, yy, yz, zz), tre_mean / tre_m2 / tre_max (K)
// float64, count (K) int32: the finite samples of the C chains folded in order (records_before == 0 overwrites)
void launch_landmark_update(const float* mapped, const float* target, int C, int K, double* mean, double* comoment, double* tre_mean,
                            double* tre_m2, double* tre_max, int32_t* count, int records_before, hipStream_t st);
// out (K, IRS_LANDMARK_COLUMNS) doubles; isummary IRS_LANDMARK_SUMMARY_INTS int64, fsummary IRS_LANDMARK_SUMMARY_FLOATS
// doubles; ws: IRS_LANDMARK_WS_BYTES (the partials of at most 1024 blocks)
void launch_landmark_finalize(const double* mean, const double* comoment, const double* tre_mean, const double* tre_m2,
                              const double* tre_max, const int32_t* count, const float* target, int K, double* out,
                              long long* isummary, double* fsummary, void* ws, hipStream_t st);

// ---- local_similarity_kernels.hip: windowed LNCC / SSIM maps and the posterior of the LNCC maps (absent in the reference)
struct LocalGeom {
    int D, H, W;
    int tiles_x, tiles;  // 32 x 8 tiles along x, and per plane
    int seg_len, nwork;  // planes per z-segment; work items = tiles x segments
    int blocks;          // blocks per chain = rows of partials per chain: min(nwork, IRS_LOCAL_MAX_BLOCKS)
};
struct LocalConsts {
    double floor_f, floor_m, c1, c2;
};
// the launch shape of a volume: depends on (D, H, W, radius) only
LocalGeom local_similarity_geometry(int D, int H, int W, int radius);
// fixed (1 or C,V) with fixed_stride 0 or V; moving (C,V); mask (V) uint8 or nullptr; lncc / ssim (C,V) or nullptr; stats (C,
// IRS_LOCAL_STATS); ws: C * g.blocks rows of 3 int64 + 4 doubles (at most IRS_LOCAL_WS_BYTES); radius in 1 .. IRS_LOCAL_MAX_RADIUS
void launch_local_similarity(const float* fixed, int64_t fixed_stride, const float* moving, const uint8_t* mask, int C, int radius,
                             const LocalGeom& g, const LocalConsts& k, float* lncc, float* ssim, double* stats, void* ws,
                             hipStream_t st);
// lncc (C,V) float32 -> mean / low (V) float32, count (V) int32: the samples that are no NaN folded in chain order
// (records_before == 0 overwrites)
void launch_local_similarity_update(const float* lncc, int C, int64_t V, float* mean, float* low, int32_t* count,
                                    int records_before, hipStream_t st);
// isummary IRS_LOCAL_MAP_SUMMARY_INTS int64, fsummary IRS_LOCAL_MAP_SUMMARY_FLOATS doubles; ws: IRS_LOCAL_MAP_WS_BYTES
void launch_local_similarity_finalize(const float* mean, const float* low, const int32_t* count, int64_t V, const uint8_t* mask,
                                      long long* isummary, double* fsummary, void* ws, hipStream_t st);

// ---- lncc_kernels.hip: the LNCC data term (squared local normalised cross-correlation over a box window) and its adjoint
struct LnccGeom {
    int D, H, W;
    int tiles_x, tiles;  // 32 x 8 tiles along x, and per plane
    int seg_len, nwork;  // planes per z-segment; work items = tiles x segments
    int blocks;          // blocks per chain = partial sums per chain: min(nwork, kMaxPartialBlocks)
};
// the launch shape of a volume: depends on (D, H, W, radius) and the `lcc_seg` switch only
LnccGeom lncc_geometry(int D, int H, int W, int radius);
// fixed (1 or C,V) with fixed_stride 0 or V; moving (C,V); u = upstream (float, stride 0 or V) if given, else mask (uint8, stride 0
// or V) if given, else 1.  d (C,V), coef (C,3,V: p, q, t) and partials ([C][g.blocks] doubles of scale * sum u d) may each be nullptr.
void launch_lncc_fwd(const float* fixed, int64_t fixed_stride, const float* moving, const float* upstream, int64_t upstream_stride,
                     const uint8_t* mask, int64_t mask_stride, int radius, float eps, double scale, float* d, float* coef,
                     double* partials, int C, const LnccGeom& g, hipStream_t st);
// g_moving (C,V) = scale * (M box^T(q) - F box^T(p) - box^T(t)) from the coefficient maps of the forward launch
void launch_lncc_bwd(const float* fixed, int64_t fixed_stride, const float* moving, const float* coef, int radius, float scale,
                     float* g_moving, int C, const LnccGeom& g, hipStream_t st);

// ---- mi_kernels.hip: the mutual-information data term (Parzen joint histogram in Q30 fixed point, the table T, the gradient)
struct MiBins {
    int bins;
    float f_lo, f_hi, f_inv;  // range of the fixed image and bins / (hi - lo), formed in fp32 (the rule of hist_bin)
    double m_lo, m_scale;     // of the moving image: m_lo and (bins - 3) / (m_hi - m_lo), formed in double
};
// blocks per chain of the accumulate and the gradient launch: min(ceil(units / 256), IRS_MI_MAX_BLOCKS / C), units of four voxels in
// the vector form
int mi_blocks(int64_t V, int C, bool vec);
// fixed (1 or C,V) with fixed_stride 0 or V; moving (C,V); mask (1 or C,V) uint8 with mask_stride 0 or V, or nullptr; hist (C,B,B)
// uint64 (zeroed on the stream here, left holding the histogram); table (C,B,B) float32; stats (C, IRS_MI_STATS); ipart:
// IRS_MI_MAX_BLOCKS rows of 3 int64; data_out (or nullptr): data_out[c * data_stride] = weight * n_c * (ln B - MI_c).  -> the status
// of the memset (nothing is launched behind one that failed)
hipError_t launch_mi_fwd(const float* fixed, int64_t fixed_stride, const float* moving, const uint8_t* mask, int64_t mask_stride, int64_t V,
                   int C, const MiBins& bn, unsigned long long* hist, float* table, double* stats, long long* ipart, double weight,
                   double* data_out, int64_t data_stride, hipStream_t st);
// g (C,V) = -weight * scale[c] * mask * inside * m_scale * sum_j w'_j T[a][k0 - 1 + j]; scale: C floats on the device or nullptr
// (1); pmi (C,V) or nullptr: sum_j w_j T[a][k0 - 1 + j] at the voxels that take part (residual_form: ln B minus that), 0 elsewhere
void launch_mi_bwd(const float* fixed, int64_t fixed_stride, const float* moving, const uint8_t* mask, int64_t mask_stride,
                   const float* table, int64_t V, int C, const MiBins& bn, float weight, const float* scale, bool residual_form,
                   float* g, float* pmi, hipStream_t st);

// ---- ngf_kernels.hip: the NGF data term (normalised gradient field distance) and its adjoint; arithmetic in ngf_device.h.  The
// launch shape is lncc_geometry(D, H, W, 1).
// fixed (1 or C,V) with fixed_stride 0 or V; moving (C,V); u = upstream (float, stride 0 or V) if given, else mask (uint8, stride 0
// or V) if given, else 1.  d (C,V; u d with weighted_map), coef (C,3,V: c_z, c_y, c_x) and partials ([C][g.blocks] doubles of
// scale * sum u d) may each be nullptr.
void launch_ngf_fwd(const float* fixed, int64_t fixed_stride, const float* moving, const float* upstream, int64_t upstream_stride,
                    const uint8_t* mask, int64_t mask_stride, float eps_f, float eps_m, double scale, bool weighted_map, float* d,
                    float* coef, double* partials, int C, const LnccGeom& g, hipStream_t st);
// g_moving (C,V) = scale * grad^T c from the coefficient maps of the forward launch
void launch_ngf_bwd(const float* coef, float scale, float* g_moving, int C, const LnccGeom& g, hipStream_t st);

// ---- residual_kernels.hip: the residuals against the mixture that models them -- histogram, moments and the per-voxel NLL
struct ResBins {
    int bins;
    float half_range, inv_w;  // bins over [-half_range, half_range]; inv_w = bins / (2 half_range), formed in fp32
};
struct ResMixture {  // passed to the kernel by value
    double log_weight[IRS_MAX_COMPONENTS];  // ln pi_k - ln sigma_k - 1/2 ln 2 pi
    double inv_std[IRS_MAX_COMPONENTS];     // 1 / sigma_k
    int K;
};
// residuals (C,V) float32; mask (V) uint8 or nullptr; hist (C,bins) / counts (C,3) int64 and sums (C,4) double, overwritten
// when records_before == 0 and added to otherwise (hist is zeroed on the stream here); ws: C * min(blocks, IRS_RESIDUAL_MAX_BLOCKS)
// rows of 3 int64 + 4 doubles (at most IRS_RESIDUAL_WS_BYTES)
void launch_residual_histogram(const float* residuals, const uint8_t* mask, int64_t V, int C, const ResBins& bn, long long* hist,
                               long long* counts, double* sums, int records_before, void* ws, hipStream_t st);
// residuals (C,V) float32 -> mean (V) float32, count (V) int32: the NLL of every finite z under `mix`, folded in chain order
// (records_before == 0 overwrites)
void launch_residual_nll_update(const float* residuals, int C, int64_t V, const ResMixture& mix, float* mean, int32_t* count,
                                int records_before, hipStream_t st);
// isummary IRS_RESIDUAL_MAP_SUMMARY_INTS int64, fsummary IRS_RESIDUAL_MAP_SUMMARY_FLOATS doubles; ws: IRS_RESIDUAL_MAP_WS_BYTES
void launch_residual_nll_finalize(const float* mean, const int32_t* count, int64_t V, const uint8_t* mask, long long* isummary,
                                  double* fsummary, void* ws, hipStream_t st);

// ---- multires_kernels.hip: the coarse-to-fine start -- `planes` volumes of the extents of `fine` <-> of `coarse` (align_corners
// grids, coarse <= fine on every axis, both >= 2); one thread per output element, grid z = planes * (first extent of the output)
void launch_restrict_image(const float* im, float* out, int planes, const Vol& fine, const Vol& coarse, hipStream_t st);
void launch_restrict_mask(const uint8_t* mask, uint8_t* out, int planes, const Vol& fine, const Vol& coarse, hipStream_t st);
void launch_prolong_field(const float* in, float* out, int planes, const Vol& coarse, const Vol& fine, hipStream_t st);

// ---- precond_kernels.hip: the adaptive pSGLD preconditioner (absent in the reference); include/irsgmcmc.h has the arithmetic
// grad_v, sigma (C, N) float32 with N = 3 D H W (sigma may be nullptr); V (N) in/out; nonfinite: one int64 on the device
void launch_precond_accumulate(const float* grad_v, const float* sigma, int C, int64_t N, float beta, float* V, long long* nonfinite,
                               hipStream_t st);
// V (3, vol) -> sigma (C, 3, vol), summary IRS_PRECOND_SUMMARY doubles; ws: precond_workspace_bytes(vol, smooth)
size_t precond_workspace_bytes(const Vol& vol, int smooth);
void launch_precond_sigma(const float* V, int C, const Vol& vol, float bias, int smooth, double damping, float sigma_min,
                          float sigma_max, const long long* nonfinite, float* sigma, double* summary, void* ws, hipStream_t st);

// ---- modes_kernels.hip: the posterior principal modes (absent in the reference); include/irsgmcmc.h has the arithmetic
// store (cap, 3, V) float32 with the new records already in slots n_before .. n_before + n_new - 1; mask (V) uint8 or nullptr;
// gram (3, cap, cap) double; ws: modes_gram_workspace_bytes(V, n_new)
size_t modes_gram_workspace_bytes(int64_t V, int n_new);
void launch_modes_gram_rows(const float* store, int cap, int n_before, int n_new, int64_t V, const uint8_t* mask, double* gram, void* ws,
                            hipStream_t st);
// coeff (M, n) double on the device, scale: three host doubles -> mean (3, V), modes (M, 3, V), explained (V) float32
void launch_modes_project(const float* store, int n, int64_t V, const double* coeff, int M, const double* scale, float* mean, float* modes,
                          float* explained, hipStream_t st);

// ---- affine_kernels.hip: the affine pre-alignment -- a map p = c + shift + lin (k - c) in voxel index coordinates, array order
struct AffineMap {  // passed to the kernels by value
    double lin[9];  // row-major
    double shift[3];
};
// fixed / moving (V) float32; mask (V) uint8 or nullptr; sums: IRS_AFFINE_SUMS doubles; partials: IRS_AFFINE_MAX_BLOCKS rows of
// IRS_AFFINE_PARTIALS doubles
void launch_affine_normal_equations(const float* fixed, const float* moving, const uint8_t* mask, const Vol& vol, const AffineMap& map,
                                    double* sums, double* partials, hipStream_t st);
// out (1,3,D,H,W): the map as a [-1,1] transformation tensor, channel 0 the last axis
void launch_affine_transformation(const AffineMap& map, float* out, const Vol& vol, hipStream_t st);
// transformation (C,3,D,H,W) in [-1,1] -> the map applied after it, as a transformation and / or a displacement in voxels (nullptr:
// not wanted)
void launch_affine_compose(const float* transformation, const AffineMap& map, float* total_transformation, float* total_displacement,
                           int C, const Vol& vol, hipStream_t st);

// ---- bspline_kernels.hip: cubic B-spline resampling of the written images (absent in the reference) -- the prefilter and the
// two gathers; include/irsgmcmc.h has the definition
// im, coeff (volumes, D,H,W) float32, coeff may be im; three launches (x, y, z); volumes * D <= 65535
void launch_bspline_prefilter(const float* im, float* coeff, int volumes, const Vol& vol, hipStream_t st);
// coeff (1 or C, V) with coeff_stride 0 or V; transformation (C,3,V) in [-1,1]; out (C,V)
void launch_bspline_warp(const float* coeff, int64_t coeff_stride, const float* transformation, float* out, int C, const Vol& vol,
                         hipStream_t st);
// the image output of launch_native_warp with the cubic rule: u (C,3,m); im, coeff (1 or C, n) with moving_stride 0 or n0 n1 n2;
// im_out (C,n)
void launch_native_warp_cubic(const float* u, const float* im, const float* coeff, int64_t moving_stride, float* im_out,
                              const NativeGeom& gm, int C, hipStream_t st);

// ---- mask_kernels.hip: foreground masks from the image (absent in the reference) -- histogram, components, selection, hole
// filling and ball morphology over C volumes of `vol`, each on its own; include/irsgmcmc.h has the definitions.  C * D <= 65535
// im (C,V); mask (1 or C, V) with mask_stride 0 or V, or nullptr; hist (C,bins) int64, zeroed on the stream here; inv_w = bins /
// (hi - lo), formed in fp32
void launch_intensity_histogram(const float* im, const uint8_t* mask, int64_t mask_stride, int64_t V, int C, float lo, float inv_w,
                                int bins, long long* hist, hipStream_t st);
void launch_mask_threshold(const float* im, float threshold, uint8_t* out, int C, const Vol& vol, hipStream_t st);
// labels (C,V) int32 and counts (C) int32 of the mask (invert: of its complement); conn 6 / 18 / 26; ws: connected_components_bytes
size_t connected_components_bytes(int C, int64_t V);
void launch_connected_components(const uint8_t* mask, bool invert, int conn, int32_t* labels, int32_t* counts, int C, const Vol& vol,
                                 void* ws, hipStream_t st);
// out may be mask; ws: mask_select_bytes
size_t mask_select_bytes(int C, int64_t V);
void launch_mask_keep_largest(const uint8_t* mask, int conn, int keep, uint8_t* out, int C, const Vol& vol, void* ws, hipStream_t st);
void launch_mask_fill_holes(const uint8_t* mask, uint8_t* out, int C, const Vol& vol, void* ws, hipStream_t st);
// the dilation by the ball of squared radius r2 (erode: of the complement, complemented); out may be mask; ws: mask_morphology_bytes
size_t mask_morphology_bytes(int C, int64_t V);
void launch_mask_dilate(const uint8_t* mask, int r2, bool erode, uint8_t* out, int C, const Vol& vol, void* ws, hipStream_t st);

// ---- scalar_kernels.hip
struct DevState;  // full definition in scalar_kernels.h
}  // namespace irs
