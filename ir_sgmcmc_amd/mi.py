"""The mutual-information data term: a Mattes-style estimator -- zero-order window on the fixed image, cubic B-spline window on the
(warped) moving image -- as two HIP operators (include/irsgmcmc.h: irs_mi_fwd, irs_mi_bwd, where the definition stands).

    MI = sum_ab p_ab T_ab,  T_ab = ln(p_ab / (p_a p_b)),  data term of a chain = weight * n * (ln B - MI) >= 0

over the n voxels where the mask is set and both intensities are finite, with the joint histogram in Q30 fixed point (uint64), so
that it is exact and two calls return the same bits.  `mi_forward` returns the table T, the statistics and, when wanted, the
histogram; `mi_backward` turns T into d(scale * n * (ln B - MI)) / d(moving) and the per-voxel pmi map; `mi_loss` is the two in a
row.  `model.loss.MI` wraps them for autograd, and the fused transition runs the same kernels with `data_loss: MI`.  Unlike every
other data term of the package MI needs no common contrast of the two images: T1 / T2, CT / MR, an inverted or folded intensity
map.  It is no per-voxel map followed by a sum: the table couples all voxels of a chain.
"""
import math

import torch

from . import _lib as L
from .ops import _as_uint8, _call, _chain_volumes, _dims5

MIN_BINS, MAX_BINS = L.IRS_MI_MIN_BINS, L.IRS_MI_MAX_BINS
STATS_COLUMNS = ('n', 'n_nonfinite', 'n_clipped', 'mi', 'h_fixed', 'h_moving', 'data_term')


def mi_ranges(fixed, moving, mask=None):
    """((f_lo, f_hi), (m_lo, m_hi)) as Python floats: the min / max of the finite values of the fixed image under its mask and of
    the moving image over the whole volume (a warp moves any of its voxels under the mask).  ONE host read-back."""
    f_ok, m_ok = torch.isfinite(fixed), torch.isfinite(moving)
    if mask is not None:
        f_ok = f_ok & (mask != 0)
    ext = torch.stack([torch.where(f_ok, fixed, math.inf).min(), torch.where(f_ok, fixed, -math.inf).max(),
                       torch.where(m_ok, moving, math.inf).min(), torch.where(m_ok, moving, -math.inf).max()]).tolist()
    return (ext[0], ext[1]), (ext[2], ext[3])


def _setup(fixed, moving, mask, bins, fixed_range, moving_range):
    if not torch.is_tensor(moving) or not torch.is_tensor(fixed):
        raise L.IrsError('fixed and moving must be tensors')
    Cn, D, H, W = _dims5(moving, 1)
    _chain_volumes('fixed', fixed, 'moving', Cn, D, H, W)
    if mask is not None:
        _chain_volumes('mask', mask, 'moving', Cn, D, H, W)
        mask = _as_uint8(mask)
    if isinstance(bins, bool) or not isinstance(bins, int) or not MIN_BINS <= bins <= MAX_BINS:
        raise L.IrsError(f'MI bins = {bins!r}, an int in {MIN_BINS}..{MAX_BINS} needed')
    if fixed_range is None or moving_range is None:
        found = mi_ranges(fixed, moving, mask)
        fixed_range = found[0] if fixed_range is None else fixed_range
        moving_range = found[1] if moving_range is None else moving_range
    ranges = [float(x) for r in (fixed_range, moving_range) for x in r]
    for name, lo, hi in (('fixed', *ranges[:2]), ('moving', *ranges[2:])):
        if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
            raise L.IrsError(f'{name} range [{lo}, {hi}]: finite bounds with hi > lo needed')
    return Cn, D, H, W, mask, ranges


def mi_forward(fixed, moving, mask=None, bins=32, fixed_range=None, moving_range=None, want_hist=False):
    """fixed (1 or C,1,D,H,W), moving (C,1,D,H,W) float32 on the GPU; mask (1 or C,1,D,H,W) bool / uint8 or None; bins in 8..64;
    fixed_range / moving_range: (lo, hi), finite with hi > lo -- None: `mi_ranges` (one host read-back; with both given the call
    does not synchronise) -> dict(table=(C,B,B) float32 [T], stats=(C,7) float64 [STATS_COLUMNS; the data term at weight 1],
    hist=(C,B,B) int64 holding the uint64 Q30 histogram, or None, ranges=[f_lo, f_hi, m_lo, m_hi]).  Two calls return the same
    bits, and chain c of a batch is the single-chain call."""
    Cn, D, H, W, mask, ranges = _setup(fixed, moving, mask, bins, fixed_range, moving_range)
    dev = moving.device
    table = torch.empty((Cn, bins, bins), device=dev, dtype=torch.float32)
    stats = torch.empty((Cn, L.IRS_MI_STATS), device=dev, dtype=torch.float64)
    hist = torch.empty((Cn, bins, bins), device=dev, dtype=torch.int64) if want_hist else None
    scratch = torch.empty(L.IRS_MI_WS_BYTES, device=dev, dtype=torch.uint8)
    _call('irs_mi_fwd', L.dev_ptr(fixed.contiguous(), torch.float32), fixed.shape[0], L.dev_ptr(moving.contiguous(), torch.float32),
          L.dev_ptr(mask, torch.uint8, True), 1 if mask is None else mask.shape[0], bins, *ranges, L.dev_ptr(hist, None, True),
          L.dev_ptr(table), L.dev_ptr(stats), L.dev_ptr(scratch), Cn, D, H, W)
    return {'table': table, 'stats': stats, 'hist': hist, 'ranges': ranges}


def mi_backward(fixed, moving, table, mask=None, bins=32, fixed_range=None, moving_range=None, scale=None, want_pmi=False):
    """d(scale_c * n * (ln B - MI)) / d(moving) (C,1,D,H,W) float32 from the table of `mi_forward` with the same images, mask, bins
    and ranges; scale: (C,) float32 on the device, or None for 1.  With want_pmi -> (gradient, pmi): pmi (C,1,D,H,W) float32, the
    pointwise mutual information sum_j w_j T[a][k0 - 1 + j] at the voxels that take part (0 elsewhere), whose sum is n MI."""
    Cn, D, H, W, mask, ranges = _setup(fixed, moving, mask, bins, fixed_range, moving_range)
    if not torch.is_tensor(table) or tuple(table.shape) != (Cn, bins, bins):
        raise L.IrsError(f'table must have shape {(Cn, bins, bins)}, got {tuple(getattr(table, "shape", ()))}')
    if scale is not None and tuple(scale.shape) != (Cn,):
        raise L.IrsError(f'scale must have shape {(Cn,)}, got {tuple(scale.shape)}')
    g = torch.empty_like(moving, memory_format=torch.contiguous_format)
    pmi = torch.empty_like(g) if want_pmi else None
    _call('irs_mi_bwd', L.dev_ptr(fixed.contiguous(), torch.float32), fixed.shape[0], L.dev_ptr(moving.contiguous(), torch.float32),
          L.dev_ptr(mask, torch.uint8, True), 1 if mask is None else mask.shape[0], L.dev_ptr(table.contiguous(), torch.float32), bins,
          *ranges, L.dev_ptr(None if scale is None else scale.contiguous(), torch.float32, True), L.dev_ptr(g), L.dev_ptr(pmi, None, True),
          Cn, D, H, W)
    return (g, pmi) if want_pmi else g


def mi_loss(fixed, moving, mask=None, bins=32, fixed_range=None, moving_range=None):
    """(n * (ln B - MI) per chain (C,) float64, its gradient with respect to moving (C,1,D,H,W) float32)"""
    out = mi_forward(fixed, moving, mask, bins, fixed_range, moving_range)
    f_lo, f_hi, m_lo, m_hi = out['ranges']
    return out['stats'][:, 6].clone(), mi_backward(fixed, moving, out['table'], mask, bins, (f_lo, f_hi), (m_lo, m_hi))
