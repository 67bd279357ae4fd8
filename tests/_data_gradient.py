"""fp64 restatement of the data-gradient stage of a transition ON ITS OWN: the mixture's d(-log p)/dz with the parameters the chain's
own Adam step left, the factor alpha, the mask and the adjoint of the LCC map (model/loss.py:53-59,102-111; trainer.py:316-330) down
to g_M = dL/d(warped image) -- what lcc_data_bwd_march_kernel writes (csrc/stencil_kernels.hip), and ssd_bwd_kernel for the SSD term.
Plain torch, float64, no GPU, formulas written out.  The boxes are small matrices: B[i, clamp(i + k)] += 1 for k = -S..S is the
replicate-padded box along one axis, and box^T is its transpose, so nothing here shares the kernel's fold-the-padding arithmetic.

g_M is no output of the library.  It is read through grad_v of a transition at velocity zero without Sobolev smoothing, jitter or
noise: the regulariser half of grad_v is then exactly 0, every squaring step's adjoint doubles its input (undone exactly by the 2^-N
prescale), the warp is the identity and its adjoint multiplies g_M by the one-sided difference of the moving image, which ATen's
border clip switches off on both faces of the channel's own axis:  grad_v[ch] = CONST g_M Delta_ch m  (tests/test_data_gradient_host.py
pins CONST and the face zeros against the oracle run in float64).  On dyadic shapes (2^k + 1 per axis) the sampling positions are
exact integers; with the triangle-wave moving image `tri_image` the differences are +-1, +-2, +-4 and max|m| = 14.

The tolerances of tests/test_gpu_data_gradient.py live here (`tol` of `data_gradient`, `tol_lcc`, the tolerance `forward` returns), derived on the reference side."""
import torch

from tests import _transition_scalars as R

F64 = torch.float64
U = 2.0 ** -24          # unit roundoff of float32
CONST = 1.0             # d grad_v / d (g_M Delta m): (n - 1)/2 of the sampler times 2/(n - 1) of to_normalised, 2^N / 2^N of the steps
DYADIC = ((9, 17, 33), (5, 9, 129), (33, 5, 65), (17, 33, 65))


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def tri(n):
    """0, 1, 2, 1, 0, 1, ..."""
    return 2 - ((torch.arange(n) % 4) - 2).abs()


def tri_image(dims):
    """tri(x) + 2 tri(y) + 4 tri(z), (1,1,D,H,W) float32: integer values 0..14, every one-sided difference +-1, +-2, +-4"""
    D, H, W = dims
    return (tri(W).view(1, 1, W) + 2 * tri(H).view(1, H, 1) + 4 * tri(D).view(D, 1, 1)).to(torch.float32).view(1, 1, D, H, W).contiguous()


def one_sided_differences(m):
    """(..., D, H, W) -> (3, ..., D, H, W): channel ch (0 <-> W, 1 <-> H, 2 <-> D) holds m[i + 1] - m[i] along its axis for
    0 < i < n - 1 and exactly 0 on both faces (the cell of an integer position i is (i, i + 1) with weights (1, 0); ATen's clip of
    the coordinate zeroes the gradient at i <= 0 and i >= n - 1)"""
    out = []
    for ax in (-1, -2, -3):
        n = m.shape[ax]
        d = torch.zeros_like(m)
        d.narrow(ax, 1, n - 2).copy_(m.narrow(ax, 2, n - 2) - m.narrow(ax, 1, n - 2))
        out.append(d)
    return torch.stack(out)


def smooth_fixed(dims, C=1, seed=11, taps=2):
    """A smooth fixed image as in make_inputs: synthetic_pair's blobs plus white noise smoothed with the Sobolev kernel of half width
    `taps` (amplitude 0.3).  The residual against the triangle-wave moving image then stays correlated from voxel to voxel, which
    keeps alpha well below 1.  Chain c of a per-chain image is rolled by 2 c rows.  -> (1 or C,1,D,H,W) float32, mask (1,1,D,H,W)"""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    from oracle import ops as O
    f, _ = synthetic_pair(dims, seed=3)
    noise = torch.randn(1, 3, *dims, generator=torch.Generator().manual_seed(seed))
    im = f['im'].unsqueeze(0) + 0.3 * O.separable_conv3d_replicate(noise, O.sobolev_kernel_1d(taps, 0.5))[:, :1]
    im = torch.cat([im.roll(2 * c, dims=-2) for c in range(C)]).to(torch.float32).contiguous()
    return im, f['mask'].unsqueeze(0).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# boxes
# ------------------------------------------------------------------------------------------------------------------------------
def box_matrix(n, s, dtype=F64):
    """B (n, n): (B x)_i = sum_{k=-s..s} x[clamp(i + k, 0, n - 1)]"""
    B = torch.zeros(n, n, dtype=dtype)
    for i in range(n):
        for k in range(-s, s + 1):
            B[i, min(max(i + k, 0), n - 1)] += 1
    return B


def apply_axis(M, x, ax):
    return torch.movedim(torch.tensordot(torch.movedim(x, ax, -1), M, dims=([-1], [1])), -1, ax)


def box(x, s):
    """(2s+1)^3 all-ones filter over clamped coordinates of the last three axes (replicate padding)"""
    for ax in (-3, -2, -1):
        x = apply_axis(box_matrix(x.shape[ax], s, x.dtype), x, ax)
    return x


def box_t(x, s, drop=(), seam=None):
    """Adjoint of `box`.  The deliberate mistakes of the host test: drop = {(axis, end)}: the extra weight of the padding that folded
    onto index 0 (end 0) or n - 1 (end 1) of axis -3 / -2 / -1 left out (every weight of that output index at most 1); seam = plane:
    outputs at and above it along D do not see the planes before it (a ring that is not primed at a segment start)."""
    for ax in (-3, -2, -1):
        n = x.shape[ax]
        M = box_matrix(n, s, x.dtype).t().clone()
        for a, end in drop:
            if a == ax:
                i = 0 if end == 0 else n - 1
                M[i] = M[i].clamp(max=1.0)
        if seam is not None and ax == -3:
            M[seam:, :seam] = 0.0
        x = apply_axis(M, x, ax)
    return x


# ------------------------------------------------------------------------------------------------------------------------------
# the LCC map and its adjoint
# ------------------------------------------------------------------------------------------------------------------------------
def lcc_stats(im, s):
    """-> (w / sigma, sigma, w): u = box(I)/n, w = I - u, var = box(w^2)/n (clamped COORDINATES: w of the volume's own voxels),
    sigma = sqrt(var + 1e-10); in the dtype of `im`"""
    n = float((2 * s + 1) ** 3)
    w = im - box(im, s) / n
    sigma = torch.sqrt(box(w * w, s) / n + 1e-10)
    return w / sigma, sigma, w


def tol_lcc(im, s):
    """How far a float32 evaluation of w / sigma may be from the float64 one, per element.  A box is an in-plane sum of (2s+1)^2 terms
    and a ring sum of 2s+1: N = (2s+1)^2 + (2s+1) + 2 roundings, each at most U x the largest partial sum, so w is off by at most
    e_w = N U max_window|I| (the window of u, 2s+1 wide).  sigma inherits e_w / sigma relative (Cauchy-Schwarz over the window of
    var, where e_w is taken at its largest: one more window) plus (N / 2 + 3) U of its own sum, square root and reciprocal.
    im: (C,1,D,H,W).  -> (tolerance of w / sigma, tolerance of sigma)"""
    k = 2 * s + 1
    N = k * k + k + 2
    im = im.to(F64)
    wh, sigma, _ = lcc_stats(im, s)
    pool = lambda x: torch.nn.functional.max_pool3d(torch.nn.functional.pad(x, (s,) * 6, mode='replicate'), k, stride=1)
    e_w = N * U * pool(im.abs())
    rel_sigma = pool(e_w) / sigma + (0.5 * N + 3.0) * U
    return e_w / sigma + wh.abs() * rel_sigma + U * wh.abs(), sigma * rel_sigma


def lcc_adjoint(g_z, wh, sigma, s, n=None, drop=(), seam=None):
    """g_M = d/dM of sum g_z z, z = fhat - w / sigma, through the formulas the kernel documents:
    pw = -g_z / sigma, gvar = -pw wh / (2 sigma), a2 = 2 wh sigma / n, ga = pw + a2 box^T(gvar), g_M = ga - box^T(ga) / n.
    -> (g_M, A): A = the sum of the absolute addends of each output, |pw| + |a2| box^T|gvar| and box^T of that over n"""
    n = float((2 * s + 1) ** 3) if n is None else float(n)
    pw = -g_z / sigma
    gvar = -0.5 * pw * wh / sigma
    a2 = (2.0 / n) * wh * sigma
    ga = pw + a2 * box_t(gvar, s, drop, seam)
    g_m = ga - box_t(ga, s, drop, seam) / n
    a_ga = pw.abs() + a2.abs() * box_t(gvar.abs(), s)
    return g_m, a_ga + box_t(a_ga, s) / n


def lcc_adjoint_autograd(g_z, fixed, moving, s):
    """the same through float64 autograd of the restated map: what `lcc_adjoint` is checked against"""
    m = moving.detach().to(F64).clone().requires_grad_(True)
    z = lcc_stats(fixed.to(F64), s)[0] - lcc_stats(m, s)[0]
    return torch.autograd.grad(z, m, g_z.to(F64))[0]


# ------------------------------------------------------------------------------------------------------------------------------
# d(-log p)/dz
# ------------------------------------------------------------------------------------------------------------------------------
def dnll_dz(z, log_std, logits, h, dtype=F64):
    """sum_k r_k z / sigma_k^2 (SSD: z / sigma^2).  float64: the responsibilities of R.mixture_eval; any other dtype: the same
    formulas carried out in it"""
    if h.data_loss != 'GMM':
        return z.to(dtype) * torch.tensor(h.ssd_inv_sigma, dtype=dtype) ** 2
    if dtype == F64:
        r = R.mixture_eval(z, log_std, logits, h)[1]
        return (r * torch.exp(-2.0 * log_std.to(F64))).sum(-1) * z.to(F64)
    ls, lg, z = log_std.to(dtype), logits.to(dtype), z.to(dtype)
    q = (z.unsqueeze(-1) * torch.exp(-ls)) ** 2
    r = torch.softmax((torch.log_softmax(lg + 1e-2, dim=0) - ls - R.LOG_SQRT_2PI) - 0.5 * q, dim=-1)
    return (r * torch.exp(-2.0 * ls)).sum(-1) * z


def dnll_dz_spread(z, log_std, logits, tol_param, h):
    """how far d(-log p)/dz moves when the 2K parameters move by their tolerance (2,K), one at a time, summed"""
    base = dnll_dz(z, log_std, logits, h)
    out = torch.zeros_like(base)
    for k in range(log_std.numel()):
        for i in range(2):
            ls, lg = log_std.to(F64).clone(), logits.to(F64).clone()
            (ls, lg)[i][k] += float(tol_param[i][k])
            out += (dnll_dz(z, ls, lg, h) - base).abs()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the stage
# ------------------------------------------------------------------------------------------------------------------------------
def chain_of(t, c):
    return t[c if t.shape[0] > 1 else 0]


def forward(fixed, moving, h, s, dtype=F64):
    """-> z (Cf,1,D,H,W) with Cf the chains of `fixed`, and its float32 tolerance (GMM: both LCC sides plus the subtraction; SSD: one
    subtraction); the moving side is the (1,1,D,H,W) moving image itself, the warp being the identity"""
    f, m = fixed.to(dtype), moving.to(dtype)
    if h.data_loss != 'GMM':
        z = f - m
        return z, U * z.abs().to(F64)
    z = lcc_stats(f, s)[0] - lcc_stats(m, s)[0]
    return z, tol_lcc(fixed, s)[0] + tol_lcc(moving, s)[0] + U * z.abs().to(F64)


def plane_distance(mask3):
    """(D,H,W) bool -> (D,1,1): how many planes each plane lies outside the mask's extent along z (0 inside it)"""
    on = mask3.flatten(1).any(1).nonzero().flatten()
    zz = torch.arange(mask3.shape[0])
    return torch.clamp(torch.maximum(int(on.min()) - zz, zz - int(on.max())), min=0).view(-1, 1, 1)


def data_gradient(z, moving, fixed, mask, alpha, params, h, s, dtype=F64, tol_params=None, n=None, drop=(), seam=None, w_from_z=False,
                  stale_map=None, no_fill=False):
    """z (C,1,D,H,W): the residual the mixture is evaluated at (the GPU's own); moving (1,1,D,H,W); fixed, mask (1 or C,1,D,H,W);
    alpha: C numbers; params: per chain (log_std, logits) in force for that chain's data term (SSD: ignored); tol_params: per chain
    the (2,K) spread of those parameters, or None.  n, drop, seam: the mistakes of box_t / lcc_adjoint.  w_from_z: w / sigma taken
    as fhat - z like the kernel does (the float32 evaluation), not from the moving image.
    The mistakes of a list-walking data stage (GMM), for a mask that leaves planes out of reach: stale_map = r: the LCC map marched
    only the planes within r of the mask's extent along z (the right reach is S) -- beyond them w / sigma and sigma are an earlier
    transition's, here those of the moving image moved by one voxel along W; no_fill: the data term did not zero-fill g_M beyond
    its reach of 2 S planes -- there g_M is an earlier transition's, here that of the mask of ones.
    -> dict g_m, A (C,1,D,H,W), grad_v, tol (C,3,D,H,W)"""
    C = z.shape[0]
    mv = moving.to(dtype)
    gms, As, Es = [], [], []
    if h.data_loss == 'GMM':
        wh_m, sigma_m, _ = lcc_stats(mv[0, 0], s)
        fhat = [lcc_stats(fixed[c, 0].to(dtype), s)[0] for c in range(fixed.shape[0])]
    for c in range(C):
        mk = chain_of(mask, c)[0].to(dtype)
        ls, lg = params[c] if params is not None else (None, None)
        g_z = float(alpha[c]) * mk * dnll_dz(z[c, 0], ls, lg, h, dtype)
        if h.data_loss != 'GMM':        # z = F - M: g_M = -g_z
            gms.append(-g_z)
            As.append(g_z.abs())
            Es.append(torch.zeros_like(g_z))
            continue
        wh = fhat[c if len(fhat) > 1 else 0] - z[c, 0].to(dtype) if w_from_z else wh_m
        sigma = sigma_m
        if stale_map is not None:
            far = plane_distance(chain_of(mask, c)[0]) > stale_map
            wh_old, sigma_old, _ = lcc_stats(mv[0, 0].roll(1, -1), s)
            wh, sigma = torch.where(far, wh_old, wh), torch.where(far, sigma_old, sigma_m)
        g_m, A = lcc_adjoint(g_z, wh, sigma, s, n, drop, seam)
        if no_fill:
            g_old = lcc_adjoint(float(alpha[c]) * dnll_dz(z[c, 0], ls, lg, h, dtype), wh, sigma, s)[0]
            g_m = torch.where(plane_distance(chain_of(mask, c)[0]) > 2 * s, g_old, g_m)
        E = torch.zeros_like(A)
        if tol_params is not None:      # the parameters are only known to their spread: that much of g_z, through the absolute map
            dg = abs(float(alpha[c])) * mk * dnll_dz_spread(z[c, 0], ls, lg, tol_params[c], h).to(dtype)
            E = lcc_adjoint(dg, wh, sigma_m, s)[1]
        gms.append(g_m)
        As.append(A)
        Es.append(E)
    g_m, A, E = torch.stack(gms).unsqueeze(1), torch.stack(As).unsqueeze(1), torch.stack(Es).unsqueeze(1)
    dm = one_sided_differences(mv[0, 0]).unsqueeze(0)                     # (1,3,D,H,W)
    grad_v = CONST * g_m * dm
    # 1e-5 of the absolute addends (the relative accuracy tol_gmm_grad grants the fast-math mixture evaluation), times the factor of the
    # read-out; plus the read-out's own rounding, the 8-tap cancellation of the warp adjoint: 8 U max|m| / |Delta m| relative
    tol = (1e-5 * A.to(F64) + E.to(F64)) * (CONST * dm).abs().to(F64) + 8.0 * U * float(mv.abs().max()) * (CONST * g_m).abs().to(F64) * (dm != 0).to(F64)
    return {'g_m': g_m, 'A': A, 'grad_v': grad_v, 'tol': tol, 'dm': dm}


def make_mask(kind, base, C):
    """The masks of tests/test_gpu_transition_scalars.py on these shapes: base (1,1,D,H,W) bool -> (1 or C,1,D,H,W) bool"""
    D, H, W = base.shape[-3:]
    zz, yy, xx = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing='ij')
    if kind == 'synthetic':
        m = base[0, 0]
    elif kind == 'checkerboard':
        m = (xx + yy + zz) % 2 == 0
    elif kind == 'seam_planes':         # the two planes on either side of the seam between the first two 4-plane segments
        m = (zz == 3) | (zz == 4)
    elif kind == 'band':                # the synthetic mask on the four planes around D / 2: planes no list of the data stage reaches
        m = base[0, 0] & (zz >= D // 2 - 2) & (zz < D // 2 + 2)
    elif kind == 'faces':               # every face of the volume on the mask
        m = base[0, 0] | (xx == 0) | (xx == W - 1) | (yy == 0) | (yy == H - 1) | (zz == 0) | (zz == D - 1)
    elif kind == 'per_chain':           # chain c's mask rolled by 3 c voxels along W
        return torch.stack([base[0].roll(3 * c, dims=-1) for c in range(C)]).contiguous()
    return m.view(1, 1, D, H, W).contiguous()


def mixture_state(fixed, moving, mask, K, s):
    """the hand-set mixture of R.hand_set_mixture with zeroed Adam moments, as the state dict of R.mixture_stage"""
    ls, lg = R.hand_set_mixture({'im': fixed, 'mask': mask}, {'im': moving}, K, s)
    return {'log_std': ls, 'logits': lg, 'm': torch.zeros(2, K), 'v': torch.zeros(2, K), 'step': [0, 0]}


def reference(z, fixed, moving, mask, h, s, state=None, alpha=None, params=None, **kw):
    """The restatement for one case, fed the residual z (C,1,D,H,W).  GMM: the serial recursion R.mixture_stage_with_spread over the
    chains gives each chain's alpha and stepped parameters with their spread; `alpha` (the GPU's own) and `params` (read back, one
    chain) replace the recursion's where given -- parameters that were read back have no spread.  -> (data_gradient dict, records)"""
    C = z.shape[0]
    recs = R.mixture_stage_with_spread(z, mask, state, h)[0] if h.data_loss == 'GMM' else R.mixture_stage(z, mask, {
        'log_std': torch.zeros(1), 'logits': torch.zeros(1), 'm': torch.zeros(2, 1), 'v': torch.zeros(2, 1), 'step': [0, 0]}, h)[0]
    alpha = [r['alpha'] for r in recs] if alpha is None else alpha
    tol_params = None
    if h.data_loss == 'GMM' and params is None:
        params = [(r['log_std'], r['logits']) for r in recs]
        tol_params = [r['tol_param'] for r in recs]
    return data_gradient(z, moving, fixed, mask, alpha, params, h, s, tol_params=tol_params, **kw), recs


def invisible_voxels(dims):
    """voxels that no channel shows: on a face of every axis -> the 8 corners"""
    dm = one_sided_differences(tri_image(dims)[0, 0])
    return int(((dm != 0).sum(0) == 0).sum())


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_data_gradient.py (tests/test_data_gradient_host.py checks on the CPU what each has to satisfy)
# ------------------------------------------------------------------------------------------------------------------------------
A, B, E, M = DYADIC
ENGINE_CASES = [
    # dims, lcc_s, C, K, mask, per-chain fixed image, config
    (A, 1, 1, 4, 'synthetic', False, {}), (A, 2, 1, 4, 'synthetic', False, {}), (B, 1, 1, 4, 'synthetic', False, {}), (B, 2, 1, 5, 'synthetic', False, {}),
    (E, 1, 1, 5, 'synthetic', False, {}), (E, 2, 1, 4, 'synthetic', False, {}), (M, 1, 1, 4, 'synthetic', False, {}), (M, 2, 1, 8, 'synthetic', False, {}),
    (A, 1, 1, 1, 'synthetic', False, {}), (A, 1, 1, 2, 'checkerboard', False, {}), (E, 2, 1, 5, 'checkerboard', False, {}),
    (B, 1, 1, 8, 'faces', False, {}), (A, 2, 1, 4, 'faces', False, {}), (A, 1, 1, 5, 'seam_planes', False, {}), (M, 2, 1, 4, 'seam_planes', False, {}),
    (A, 1, 1, 4, 'synthetic', False, {'virtual_decimation': False}), (B, 2, 1, 5, 'faces', False, {'virtual_decimation': False}),
    (A, 1, 3, 4, 'per_chain', True, {}), (M, 2, 3, 5, 'per_chain', False, {}), (B, 2, 3, 8, 'synthetic', True, {}), (E, 1, 3, 2, 'faces', True, {'virtual_decimation': False}),
    (A, 1, 2, 1, 'synthetic', False, {'data_loss': 'SSD'}), (B, 1, 2, 1, 'faces', True, {'data_loss': 'SSD', 'virtual_decimation': False}),
    (M, 1, 1, 1, 'per_chain', False, {'data_loss': 'SSD'}),
]


# (K = 2: the hand-set mixture's narrow component makes the rescaled residual so heavy-tailed that every lag correlation sits below
# exp(-pi/2) and alpha is capped at exactly 1 -- those cases run without virtual decimation or on the checkerboard, where alpha = 1 is
# the configuration's and not an accident that would hide a missing alpha)


# The list-walking kernels of the sparse data stage (lcc_fwd_march_plan_kernel, lcc_data_bwd_march_plan_kernel) against the same
# restatement: masks confined to a few planes, so that the lists leave planes unmarched on shapes this small, with pieces of
# SPARSE_PIECE planes, so that D = 17 and D = 33 get seams inside a run range.
SPARSE_PIECE = 4
SPARSE_CASES = [
    (E, 1, 1, 4, 'band', False, {}), (E, 2, 1, 5, 'band', False, {}), (M, 1, 1, 8, 'band', False, {}), (M, 2, 1, 4, 'band', False, {}),
    (E, 2, 1, 8, 'seam_planes', False, {}), (M, 1, 1, 5, 'seam_planes', False, {}),
    (E, 2, 1, 4, 'band', False, {'virtual_decimation': False}), (M, 1, 1, 5, 'band', False, {'virtual_decimation': False}),
    (E, 1, 3, 4, 'band', True, {}), (M, 2, 3, 5, 'seam_planes', True, {}), (M, 2, 3, 8, 'band', True, {'virtual_decimation': False}),
]


def case_id(c):
    return '-'.join(['x'.join(map(str, c[0]))] + [str(x) if not isinstance(x, dict) else ','.join(f'{k}={v}' for k, v in x.items()) for x in c[1:]]).rstrip('-')


def case_inputs(dims, C, mask_kind, per_chain_fixed):
    """-> fixed (1 or C,1,D,H,W), moving (1,1,D,H,W), mask (1 or C,1,D,H,W)"""
    fixed, base = smooth_fixed(dims, C if per_chain_fixed else 1)
    return fixed, tri_image(dims), make_mask(mask_kind, base, C)
