"""The LNCC data term: VoxelMorph's squared local normalised cross-correlation over a (2 radius + 1)^3 box window with clamped
indices, as two HIP operators (include/irsgmcmc.h: irs_lncc_fwd, irs_lncc_bwd), all of it float32.

    A = S_fm - S_f S_m / n,  Bf = S_ff - S_f^2 / n,  Bm = S_mm - S_m^2 / n,  d = 1 - A^2 / (Bf Bm + eps)

`lncc_forward` returns the map d, the coefficient maps of its gradient and sum u d per chain; `lncc_backward` turns the
coefficient maps into d(sum u d)/d(moving); `lncc_loss` is the two in a row.  `model.loss.LNCC` wraps them for autograd, and
the fused transition runs the same two kernels with `data_loss: LNCC`.  Unlike the mixture's pointwise residual the term does
not change under a local gain or offset of either image.  The images should be scaled to O(1): the variances are differences
of float32 window sums.
"""
import torch

from . import _lib as L
from .ops import _call, _chain_volumes, _dims5

MAX_RADIUS = L.IRS_MAX_HALF_WIDTH


def _images(fixed, moving, radius):
    if not torch.is_tensor(moving) or not torch.is_tensor(fixed):
        raise L.IrsError('fixed and moving must be tensors')
    Cn, D, H, W = _dims5(moving, 1)
    _chain_volumes('fixed', fixed, 'moving', Cn, D, H, W)
    if not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
        raise L.IrsError(f'LNCC radius = {radius!r}, an int in 1..{MAX_RADIUS} needed')
    if min(D, H, W) < 2 * radius + 1:
        raise L.IrsError(f'dims ({D}, {H}, {W}), every one >= 2 radius + 1 = {2 * radius + 1} needed')
    return Cn, D, H, W


def lncc_forward(fixed, moving, radius=2, eps=1e-5, upstream=None, want_map=True, want_coef=True, want_sums=True):
    """fixed (1 or C,1,D,H,W), moving (C,1,D,H,W), upstream u None (= 1) or (1 or C,1,D,H,W), float32 on the GPU ->
    dict(d=(C,1,D,H,W) float32, coef=(C,3,D,H,W) float32 [p, q, t], sums=(C,) float64 [sum u d]); what is not wanted is None.
    Two calls return the same bits, and chain c of a batch is the single-chain call."""
    Cn, D, H, W = _images(fixed, moving, radius)
    if not (eps > 0.0 and eps < float('inf')):
        raise L.IrsError(f'eps = {eps!r}, a finite value > 0 needed')
    if upstream is not None:
        _chain_volumes('upstream', upstream, 'moving', Cn, D, H, W)
    dev = moving.device
    d = torch.empty_like(moving, memory_format=torch.contiguous_format) if want_map else None
    coef = torch.empty((Cn, 3, D, H, W), device=dev, dtype=torch.float32) if want_coef else None
    sums = torch.empty(Cn, device=dev, dtype=torch.float64) if want_sums else None
    scratch = torch.empty(L.load().irs_reduce_scratch_doubles(), device=dev, dtype=torch.float64) if want_sums else None
    _call('irs_lncc_fwd', L.dev_ptr(fixed.contiguous(), torch.float32), fixed.shape[0], L.dev_ptr(moving.contiguous(), torch.float32),
          L.dev_ptr(None if upstream is None else upstream.contiguous(), torch.float32, allow_none=True),
          1 if upstream is None else upstream.shape[0], radius, float(eps), L.dev_ptr(d, None, True), L.dev_ptr(coef, None, True),
          L.dev_ptr(sums, None, True), L.dev_ptr(scratch, None, True), Cn, D, H, W)
    return {'d': d, 'coef': coef, 'sums': sums}


def lncc_backward(fixed, moving, coef, radius=2):
    """d(sum u d)/d(moving) (C,1,D,H,W) float32 from the coefficient maps `coef` (C,3,D,H,W) of `lncc_forward` with the same
    fixed, moving and radius"""
    Cn, D, H, W = _images(fixed, moving, radius)
    if not torch.is_tensor(coef) or tuple(coef.shape) != (Cn, 3, D, H, W):
        raise L.IrsError(f'coef must have shape {(Cn, 3, D, H, W)}, got {tuple(getattr(coef, "shape", ()))}')
    g = torch.empty_like(moving, memory_format=torch.contiguous_format)
    _call('irs_lncc_bwd', L.dev_ptr(fixed.contiguous(), torch.float32), fixed.shape[0], L.dev_ptr(moving.contiguous(), torch.float32),
          L.dev_ptr(coef.contiguous(), torch.float32), radius, L.dev_ptr(g), Cn, D, H, W)
    return g


def lncc_loss(fixed, moving, radius=2, eps=1e-5, upstream=None):
    """(sum u d per chain (C,) float64, its gradient with respect to moving (C,1,D,H,W) float32)"""
    out = lncc_forward(fixed, moving, radius, eps, upstream, want_map=False)
    return out['sums'], lncc_backward(fixed, moving, out['coef'], radius)
