"""Affine pre-alignment: a rigid or affine map of the pair estimated on the device before the chains start, and the
`trainer.affine_init` option.

Conventions (include/irsgmcmc.h, "Affine pre-alignment"): voxel index coordinates in array order (D, H, W),
centre c = ((D - 1) / 2, (H - 1) / 2, (W - 1) / 2); a map is `lin` (3 x 3) and `shift` (3), numpy float64, and fixed voxel k reads
the moving image at p = c + shift + lin (k - c).  The hot path is one HIP reduction (irs_affine_normal_equations): one pass over
the volumes gathers the moving image and its gradient, forms the residual and reduces the Gauss-Newton normal equations in
double.  Levenberg-Marquardt on the host solves the 12 x 12 system, or the 6 x 6 one of a rigid map, per iteration.  The moving
triple is resampled through the map once with the package's own warps, and a sampled transformation phi composes with the map
A to the total x -> A(phi(x)) (irs_affine_compose).

The operator wrappers live here and not in ops.py; they use its helpers.
"""
import ctypes as C
import numbers

import numpy as np
import torch

from . import _lib as L
from . import multires, ops
from .ops import _call

KINDS = {'rigid': 6, 'affine': 12}
MIN_EXTENT = multires.MIN_EXTENT
MAX_LEVELS = multires.MAX_LEVELS
OPTION_KEYS = ('model', 'levels', 'max_iters', 'tol', 'min_overlap')
DEFAULTS = {'levels': (), 'max_iters': 50, 'tol': 1e-3, 'min_overlap': 0.5}


# ---------------------------------------------------------------- the operators
def _map(lin, shift):
    """(lin, shift) as float64 arrays of (3,3) and (3,), refused when they have another shape"""
    lin, shift = np.asarray(lin, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    if lin.shape != (3, 3) or shift.shape != (3,):
        raise L.IrsError(f'a map is lin (3,3) and shift (3,), got {lin.shape} and {shift.shape}')
    return np.ascontiguousarray(lin), np.ascontiguousarray(shift)


def _map_args(lin, shift):
    lin, shift = _map(lin, shift)
    return (C.c_double * 9)(*lin.reshape(-1).tolist()), (C.c_double * 3)(*shift.tolist())


def _volume(name, t):
    """a (D,H,W) volume, whatever its leading dimensions of 1 -> (D, H, W)"""
    if t.dim() < 3 or t.numel() != t.shape[-3] * t.shape[-2] * t.shape[-1]:
        raise L.IrsError(f'{name} must be one (D,H,W) volume, got {tuple(t.shape)}')
    return tuple(int(n) for n in t.shape[-3:])


def normal_equations(fixed, moving, mask, lin, shift):
    """fixed, moving: one float32 volume each ((D,H,W) or (1,1,D,H,W)); mask: bool / uint8 of the same extents or None ->
    {'H': (12,12) symmetric, 'b': (12,), 'ssd', 'n', 'n_outside', 'n_nonfinite'}, numpy float64 and ints: the Gauss-Newton
    normal equations of sum r^2, r = M(p) - F(k), in theta = (lin row-major, shift) (irs_affine_normal_equations).
    Reads the 94 doubles back: one host synchronisation per call -- the solver on the host needs them, and the stage runs some
    tens of times per run."""
    D, H, W = _volume('fixed', fixed)
    if _volume('moving', moving) != (D, H, W):
        raise L.IrsError(f'moving shape {tuple(moving.shape)} does not match fixed {tuple(fixed.shape)}')
    m = ops._volume_mask(mask, D, H, W)
    a, s = _map_args(lin, shift)
    sums = torch.empty(L.IRS_AFFINE_SUMS, device=fixed.device, dtype=torch.float64)
    ws = torch.empty(L.IRS_AFFINE_WS_BYTES, device=fixed.device, dtype=torch.uint8)
    _call('irs_affine_normal_equations', L.dev_ptr(fixed.contiguous(), torch.float32), L.dev_ptr(moving.contiguous(), torch.float32),
          L.dev_ptr(m, torch.uint8, True), D, H, W, a, s, L.dev_ptr(sums), L.dev_ptr(ws), L.IRS_AFFINE_WS_BYTES)
    return unpack_sums(sums.cpu().numpy())


def unpack_sums(v):
    """the IRS_AFFINE_SUMS doubles of the header -> the dict of normal_equations"""
    Hm = np.zeros((12, 12))
    Hm[np.triu_indices(12)] = v[:78]
    Hm = Hm + np.triu(Hm, 1).T
    return {'H': Hm, 'b': np.array(v[78:90]), 'ssd': float(v[90]), 'n': int(v[91]), 'n_outside': int(v[92]),
            'n_nonfinite': int(v[93])}


def affine_transformation(lin, shift, dims, device='cuda:0'):
    """the map as the (1,3,D,H,W) float32 transformation tensor in [-1,1] that ops.warp takes (component 0 = x, the last
    axis; irs_affine_transformation).  No host synchronisation."""
    D, H, W = multires._extents('dims', dims)
    a, s = _map_args(lin, shift)
    out = torch.empty((1, 3, D, H, W), device=device, dtype=torch.float32)
    _call('irs_affine_transformation', a, s, L.dev_ptr(out), D, H, W)
    return out


def compose(transformation, lin, shift):
    """transformation (C,3,D,H,W) float32 in [-1,1], the sampled map phi on the pair resampled through A = (lin, shift) ->
    (total_transformation in [-1,1], total_displacement in voxels), both (C,3,D,H,W), of x -> A(phi(x)) (irs_affine_compose).
    No host synchronisation."""
    Cn, D, H, W = ops._dims5(transformation, 3)
    a, s = _map_args(lin, shift)
    total_t, total_d = torch.empty_like(transformation), torch.empty_like(transformation)
    _call('irs_affine_compose', L.dev_ptr(transformation, torch.float32), a, s, L.dev_ptr(total_t), L.dev_ptr(total_d), Cn, D, H, W)
    return total_t, total_d


def is_identity(lin, shift):
    lin, shift = _map(lin, shift)
    return bool(np.array_equal(lin, np.eye(3)) and not shift.any())


def resample_pair(moving, lin, shift):
    """moving {'im', 'mask', 'seg'} of (1,1,D,H,W) (any subset) -> the same keys on the fixed grid: every volume read at
    p = c + shift + lin (k - c) through ops.warp (float32 trilinear, bool / int16 nearest, border padding), dtypes kept.
    The exact identity map returns copies: a float32 [-1,1] grid cannot place every node of a general extent exactly, and there
    is nothing to resample."""
    if is_identity(lin, shift):
        return {k: v.clone() for k, v in moving.items()}
    out, t = {}, None
    for key, vol in moving.items():
        if vol.dim() != 5 or vol.shape[:2] != (1, 1):
            raise L.IrsError(f'moving[{key!r}] must have shape (1,1,D,H,W), got {tuple(vol.shape)}')
        if t is None:
            t = affine_transformation(lin, shift, vol.shape[2:], vol.device)
        out[key] = ops.warp(vol.contiguous(), t)
    return out


# ---------------------------------------------------------------- matrices in other coordinates (all in array order)
def centre(dims):
    return (np.asarray(dims, dtype=np.float64) - 1.0) / 2.0


def _homogeneous(A, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = A, t
    return M


def index_matrix(lin, shift, dims):
    """4 x 4 matrix M with p = M (k, 1) in voxel index coordinates"""
    lin, shift = _map(lin, shift)
    c = centre(dims)
    return _homogeneous(lin, c + shift - lin @ c)


def from_index_matrix(M, dims):
    M, c = np.asarray(M, dtype=np.float64), centre(dims)
    return M[:3, :3].copy(), M[:3, 3] - c + M[:3, :3] @ c


def normalised_matrix(lin, shift, dims):
    """4 x 4 matrix of the map in the [-1,1] coordinates u_a = 2 k_a / (n_a - 1) - 1 (array order: u_0 along D)"""
    lin, shift = _map(lin, shift)
    h = centre(dims)  # (n - 1) / 2: u = (k - c) / h
    return _homogeneous(lin * h[None, :] / h[:, None], shift / h)


def from_normalised_matrix(M, dims):
    M, h = np.asarray(M, dtype=np.float64), centre(dims)
    return M[:3, :3] * h[:, None] / h[None, :], M[:3, 3] * h


def mm_matrix(lin, shift, dims, spacing):
    """4 x 4 matrix of the map in millimetres x = spacing * k (origin at voxel 0, array order)"""
    s = np.asarray(spacing, dtype=np.float64)
    M = index_matrix(lin, shift, dims)
    return _homogeneous(M[:3, :3] * s[:, None] / s[None, :], M[:3, 3] * s)


def from_mm_matrix(M, dims, spacing):
    M, s = np.asarray(M, dtype=np.float64), np.asarray(spacing, dtype=np.float64)
    return from_index_matrix(_homogeneous(M[:3, :3] * s[None, :] / s[:, None], M[:3, 3] / s), dims)


def carry_map(lin, shift, from_dims, to_dims):
    """the same map on another align_corners grid of the same field of view: with rho_a = (n_a - 1) / (N_a - 1), n of
    `to_dims` and N of `from_dims`, lin -> diag(rho) lin diag(rho)^-1 and shift -> rho shift"""
    lin, shift = _map(lin, shift)
    rho = (np.asarray(to_dims, dtype=np.float64) - 1.0) / (np.asarray(from_dims, dtype=np.float64) - 1.0)
    return lin * rho[:, None] / rho[None, :], shift * rho


# ---------------------------------------------------------------- the model
def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _rodrigues_terms(t2):
    """A = sin t / t, B = (1 - cos t) / t^2 and A' = (dA/dt) / t, B' = (dB/dt) / t at t^2 = t2; series below t = 1e-2"""
    if t2 < 1e-4:
        return (1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0,
                -1.0 / 3.0 + t2 / 30.0 - t2 * t2 / 840.0, -1.0 / 12.0 + t2 / 180.0 - t2 * t2 / 6720.0)
    t = np.sqrt(t2)
    s, c = np.sin(t), np.cos(t)
    return s / t, (1.0 - c) / t2, (t * c - s) / (t * t2), (t * s - 2.0 * (1.0 - c)) / (t2 * t2)


def rotation(omega):
    """Rodrigues: the rotation about omega / |omega| by |omega| radians"""
    w = np.asarray(omega, dtype=np.float64)
    A, B, _, _ = _rodrigues_terms(float(w @ w))
    K = _skew(w)
    return np.eye(3) + A * K + B * (K @ K)


def rotation_jacobian(omega):
    """(3,3,3): [i] = dR / d omega_i"""
    w = np.asarray(omega, dtype=np.float64)
    A, B, dA, dB = _rodrigues_terms(float(w @ w))
    K = _skew(w)
    K2 = K @ K
    out = np.empty((3, 3, 3))
    for i in range(3):
        Ki = _skew(np.eye(3)[i])
        out[i] = A * Ki + B * (Ki @ K + K @ Ki) + w[i] * (dA * K + dB * K2)
    return out


class AffineModel:
    """kind "affine": theta = (lin row-major, shift), 12 parameters, identity at (I, 0).
    kind "rigid": theta = (omega, shift), 6 parameters: rigid in MILLIMETRES, lin = S^-1 R(omega) S with S = diag(spacing) in
    array order and R the Rodrigues rotation of the rotation vector omega; the shift is in voxels."""

    def __init__(self, kind, spacing=(1.0, 1.0, 1.0)):
        if kind not in KINDS:
            raise ValueError(f'an affine model is one of {sorted(KINDS)}, got {kind!r}')
        s = np.asarray(spacing, dtype=np.float64).reshape(-1)
        if s.shape != (3,) or not np.all(np.isfinite(s)) or not np.all(s > 0):
            raise ValueError(f'spacing must hold three finite numbers > 0, got {spacing!r}')
        self.kind, self.spacing, self.n = kind, s, KINDS[kind]

    def identity(self):
        return np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]) if self.kind == 'affine' else np.zeros(6)

    def matrix(self, theta):
        """theta -> (lin, shift)"""
        theta = np.asarray(theta, dtype=np.float64)
        if theta.shape != (self.n,):
            raise ValueError(f'a {self.kind} map has {self.n} parameters, got {theta.shape}')
        if self.kind == 'affine':
            return theta[:9].reshape(3, 3).copy(), theta[9:].copy()
        s = self.spacing
        return rotation(theta[:3]) * s[None, :] / s[:, None], theta[3:].copy()

    def jacobian(self, theta):
        """(12, n): d (lin row-major, shift) / d theta"""
        if self.kind == 'affine':
            return np.eye(12)
        theta = np.asarray(theta, dtype=np.float64)
        s = self.spacing
        P = np.zeros((12, 6))
        dR = rotation_jacobian(theta[:3])
        for i in range(3):
            P[:9, i] = (dR[i] * s[None, :] / s[:, None]).reshape(-1)
        P[9:, 3:] = np.eye(3)
        return P

    def from_map(self, lin, shift):
        """the parameters of a map of this model (rigid: the rotation nearest to S lin S^-1)"""
        lin, shift = _map(lin, shift)
        if self.kind == 'affine':
            return np.concatenate([lin.reshape(-1), shift])
        s = self.spacing
        U, _, Vt = np.linalg.svd(lin * s[:, None] / s[None, :])
        R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
        cos = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
        angle = np.arccos(cos)
        axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        norm = np.linalg.norm(axis)
        omega = axis * (angle / norm) if norm > 1e-12 else axis / 2.0
        return np.concatenate([omega, shift])

    def at_level(self, from_dims, to_dims):
        """the model of the same field of view sampled on `to_dims`: the voxels grow by (N - 1) / (n - 1)"""
        rho = (np.asarray(to_dims, dtype=np.float64) - 1.0) / (np.asarray(from_dims, dtype=np.float64) - 1.0)
        return AffineModel(self.kind, self.spacing / rho)


# ---------------------------------------------------------------- Levenberg-Marquardt
def box_corners(mask, dims):
    """the eight corners of the bounding box of a mask (numpy bool (D,H,W), or None: the whole grid) -> (8,3) float64"""
    lo, hi = np.zeros(3), np.asarray(dims, dtype=np.float64) - 1.0
    if mask is not None and mask.any():
        idx = np.nonzero(mask)
        lo, hi = np.array([i.min() for i in idx], dtype=np.float64), np.array([i.max() for i in idx], dtype=np.float64)
    return np.array([[(lo, hi)[(j >> a) & 1][a] for a in range(3)] for j in range(8)])


def corner_motion(a, b, corners, dims):
    """the largest distance, in voxels, between the images of the corners under the maps a and b"""
    d = corners - centre(dims)
    return float(np.linalg.norm(d @ (a[0] - b[0]).T + (a[1] - b[1]), axis=1).max())


def levenberg_marquardt(normal_eq, model, theta, corners, dims, n_masked, max_iters=50, tol=1e-3, min_overlap=0.5):
    """Levenberg-Marquardt on the mean squared residual ssd / n with Marquardt's diag(H) damping.
    normal_eq(lin, shift) -> the dict of normal_equations: the device operator, or any restatement of it.  A trial step is
    accepted when its n is at least min_overlap * n_masked and its ssd / n is smaller; the damping falls tenfold on an
    accepted and rises tenfold on a rejected step.  Stops when an accepted step moves no corner by more than `tol` voxels,
    after `max_iters` trial steps, or when the damping has left [1e-12, 1e12].  -> (theta, history)"""
    theta = np.asarray(theta, dtype=np.float64).copy()
    here = normal_eq(*model.matrix(theta))
    if here['n'] < max(1, min_overlap * n_masked):
        raise ValueError(f'affine pre-alignment: the start map leaves {here["n"]} of {n_masked} masked voxels inside the moving image, '
                         f'fewer than min_overlap = {min_overlap:g} of them')
    hist = {'dims': tuple(int(n) for n in dims), 'iterations': 0, 'accepted': 0, 'mean_ssd_first': here['ssd'] / here['n'],
            'converged': False}
    lam = 1e-3
    while hist['iterations'] < max_iters and 1e-12 <= lam <= 1e12:
        hist['iterations'] += 1
        P = model.jacobian(theta)
        Hr, br = P.T @ here['H'] @ P, P.T @ here['b']
        diag = np.diag(Hr).copy()
        diag[diag <= 0] = diag.max() * 1e-12 if diag.max() > 0 else 1.0
        try:
            step = np.linalg.solve(Hr + lam * np.diag(diag), -br)
        except np.linalg.LinAlgError:
            lam *= 10.0
            continue
        trial = theta + step
        there = normal_eq(*model.matrix(trial))
        if there['n'] >= max(1, min_overlap * n_masked) and there['ssd'] / there['n'] < here['ssd'] / here['n']:
            moved = corner_motion(model.matrix(trial), model.matrix(theta), corners, dims)
            theta, here, lam = trial, there, max(lam / 10.0, 1e-12)
            hist['accepted'] += 1
            if moved <= tol:
                hist['converged'] = True
                break
        else:
            lam *= 10.0
    hist.update(mean_ssd_last=here['ssd'] / here['n'], overlap=here['n'] / max(n_masked, 1))
    return theta, hist


def _standardise(fixed_im, moving_im, mask):
    """both images through ONE map (x - mean) / std, the mean and the standard deviation taken over the masked finite values
    of the two unaligned images together: the same intensity map on both sides leaves the minimiser where it is (each image by
    its own statistics would not: the mask covers other tissue in the unaligned moving image) and makes the residuals, and
    with them `tol` and the logged SSD, independent of the scanner's units.  torch reductions: plumbing."""
    pick = (lambda im: im[mask]) if mask is not None else (lambda im: im.reshape(-1))
    sel = torch.cat([pick(fixed_im), pick(moving_im)])
    sel = sel[torch.isfinite(sel)].double()
    mean, std = (float(sel.mean()), float(sel.std())) if sel.numel() > 1 else (0.0, 1.0)
    std = std if std > 0 else 1.0
    return tuple(((im.double() - mean) / std).float().contiguous() for im in (fixed_im, moving_im))


def register(fixed_im, moving_im, mask, model, levels=(), max_iters=50, tol=1e-3, min_overlap=0.5,
             normal_eq=normal_equations, log=None):
    """fixed_im, moving_im (1,1,D,H,W) float32 on the device, mask (1,1,D,H,W) bool / uint8 or None, model an AffineModel with
    the spacing of the full grid -> (lin, shift, history): the map on the full grid that minimises the mean squared
    difference of the standardised pair over the mask, and one history dict per level ({'dims', 'iterations', 'accepted',
    'mean_ssd_first', 'mean_ssd_last', 'overlap', 'converged'}).  Both images are standardised once by the masked mean and
    standard deviation of the unaligned pair (_standardise).  `levels`: grids coarser than the full one, coarse to fine; the pair is restricted to each
    (multires.restrict_image / restrict_mask, always from the full grid), the map is carried from level to level (carry_map)
    and the full grid comes last.  normal_eq(fixed, moving, mask, lin, shift): the operator; the tests pass a restatement."""
    dims = tuple(int(n) for n in fixed_im.shape[2:])
    bmask = None if mask is None else mask.bool()
    f, m = _standardise(fixed_im, moving_im, bmask)
    theta, prev, history = model.identity(), dims, []
    for level in [tuple(int(n) for n in lv) for lv in levels] + [dims]:
        if level == dims:
            fl, ml, kl = f, m, bmask
        else:
            fl, ml = multires.restrict_image(f, level), multires.restrict_image(m, level)
            kl = None if bmask is None else multires.restrict_mask(bmask, level)
        level_model = model.at_level(dims, level)
        theta = level_model.from_map(*carry_map(*model.at_level(dims, prev).matrix(theta), prev, level))
        host_mask = None if kl is None else kl[0, 0].cpu().numpy()
        n_masked = int(np.prod(level)) if host_mask is None else int(host_mask.sum())
        theta, hist = levenberg_marquardt(lambda lin, shift: normal_eq(fl, ml, kl, lin, shift), level_model, theta,
                                          box_corners(host_mask, level), level, n_masked, max_iters, tol, min_overlap)
        history.append(hist)
        if log is not None:
            log(f'affine pre-alignment ({model.kind}) at {list(level)}: {hist["iterations"]} iterations, {hist["accepted"]} accepted, '
                f'mean SSD {hist["mean_ssd_first"]:.6g} -> {hist["mean_ssd_last"]:.6g}, overlap {hist["overlap"]:.4f}'
                f'{"" if hist["converged"] else " (not converged)"}')
        prev = level
    lin, shift = model.matrix(theta)
    return lin, shift, history


# ---------------------------------------------------------------- the option
def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def affine_init_options(cfg_trainer, fine_dims):
    """`trainer.affine_init = {"model": "rigid" | "affine", "levels": [[d, h, w], ...], "max_iters": n, "tol": voxels,
    "min_overlap": fraction}` -> None when absent / null / false, else {'model', 'levels': ((d, h, w), ...), 'max_iters', 'tol',
    'min_overlap'} with the defaults filled in.  All keys but "model" are optional.  Refuses unknown keys, another model, more
    than MAX_LEVELS levels, a level that is not three integers, has an extent below MIN_EXTENT, exceeds the next level or the
    full grid on some axis or is the full grid, max_iters < 1, tol <= 0, min_overlap outside (0, 1], and the combination with
    trainer.native_resolution or trainer.landmarks: both address the moving image's own voxel space, which the pre-alignment
    does not carry through (out of scope: DESIGN.md section 6)."""
    what = 'trainer.affine_init'
    opt = cfg_trainer.get('affine_init')
    if opt is None or opt is False:
        return None
    if not isinstance(opt, dict):
        raise ValueError(f'{what} must be {{"model": "rigid" | "affine", ...}} with the optional keys {list(OPTION_KEYS[1:])}, got {opt!r}')
    unknown = set(opt) - set(OPTION_KEYS)
    if unknown:
        raise ValueError(f'{what}: unknown keys {sorted(unknown)}; known: {list(OPTION_KEYS)}')
    if opt.get('model') not in KINDS:
        raise ValueError(f'{what}.model must be one of {sorted(KINDS)}, got {opt.get("model")!r}')
    for other in ('native_resolution', 'landmarks'):
        if cfg_trainer.get(other):
            raise ValueError(f'{what} cannot be combined with trainer.{other}: it addresses the moving image\'s own voxel space, '
                             f'which the pre-alignment resamples away and does not carry through')
    out = {**DEFAULTS, **opt}
    if not _is_int(out['max_iters']):
        raise ValueError(f'{what}.max_iters must be an integer, got {out["max_iters"]!r}')
    if out['max_iters'] < 1:
        raise ValueError(f'{what}: max_iters must be >= 1, got {out["max_iters"]}')
    for key, ok, need in (('tol', lambda v: v > 0 and v != float('inf'), 'a finite number > 0'),
                          ('min_overlap', lambda v: 0 < v <= 1, 'a number in (0, 1]')):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not ok(v):
            raise ValueError(f'{what}.{key} must be {need}, got {v!r}')
        out[key] = float(v)
    levels = out['levels']
    if not isinstance(levels, (list, tuple)) or len(levels) > MAX_LEVELS:
        raise ValueError(f'{what}.levels must be a list of at most {MAX_LEVELS} levels [d, h, w], got {levels!r}')
    fine = tuple(int(n) for n in fine_dims)
    for i, dims in enumerate(levels):
        if not isinstance(dims, (list, tuple)) or len(dims) != 3 or not all(_is_int(n) for n in dims):
            raise ValueError(f'{what}.levels[{i}] must be three integers [d, h, w], got {dims!r}')
        if min(dims) < MIN_EXTENT:
            raise ValueError(f'{what}.levels[{i}]: dims {list(dims)} have an extent below {MIN_EXTENT}')
        above, name = (levels[i + 1], f'levels[{i + 1}]') if i + 1 < len(levels) else (fine, 'the full grid')
        if isinstance(above, (list, tuple)) and len(above) == 3 and all(_is_int(n) for n in above) and any(a > b for a, b in zip(dims, above)):
            raise ValueError(f'{what}.levels[{i}]: dims {list(dims)} exceed {list(above)} of {name}')
    if levels and tuple(levels[-1]) == fine:
        raise ValueError(f'{what}.levels[{len(levels) - 1}]: dims {list(fine)} are the full grid; the last level must be coarser')
    out['levels'] = tuple(tuple(int(n) for n in dims) for dims in levels)
    out['max_iters'] = int(out['max_iters'])
    return out
