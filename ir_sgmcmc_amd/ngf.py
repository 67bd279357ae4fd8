"""The NGF data term: the normalised gradient field distance of Haber & Modersitzki (2006) as two HIP operators
(include/irsgmcmc.h: irs_ngf_fwd, irs_ngf_bwd, where the definition stands), all of it float32.

    a = grad F,  b = grad M,  d = 1 - (a.b)^2 / ((|a|^2 + eps_f^2) (|b|^2 + eps_m^2))   in [0, 1]

with clamped central differences.  It compares only the direction of the two image gradients, and not their sign: it is local
like LNCC and needs no common contrast like MI, so an inverted pair under a smooth intensity inhomogeneity still registers.
`ngf_forward` returns the map d, the coefficient maps c = u dd/db of its gradient and sum u d per chain; `ngf_backward` turns
the coefficient maps into d(sum u d)/d(moving) = grad^T c; `ngf_loss` is the two in a row.  `model.loss.NGF` wraps them for
autograd, and the fused transition runs the same two kernels with `data_loss: NGF`.  Every operation is rounded once in a fixed
order, so a numpy float32 restatement reproduces all three outputs bit for bit.  `ngf_edge_parameters` is Haber's automatic
choice of the two edge parameters.
"""
import math

import torch

from . import _lib as L
from .ops import _call, _chain_volumes, _dims5


def _positive(name, value):
    value = float(value)
    if not (value > 0.0 and math.isfinite(value)):
        raise L.IrsError(f'{name} = {value!r}, a finite value > 0 needed')
    return value


def image_gradient(im):
    """the central difference with clamped indices, in voxel units, on the last three axes: (..., D, H, W) -> three tensors (z, y, x)
    of the same shape, in the dtype of `im`.  Plain torch: not hot."""
    out = []
    for ax in (-3, -2, -1):
        n = im.shape[ax]
        i = torch.arange(n, device=im.device)
        out.append(0.5 * (im.index_select(ax, (i + 1).clamp(max=n - 1)) - im.index_select(ax, (i - 1).clamp(min=0))))
    return out


def ngf_edge_parameters(fixed, moving, fixed_mask=None, moving_mask=None):
    """(eps_f, eps_m) as Python floats: each the mean of |grad I| over the image's mask (the whole volume without one), the automatic
    choice of Haber & Modersitzki.  A float64 torch reduction; ONE host read-back."""
    eps = []
    for im, mask in ((fixed, fixed_mask), (moving, moving_mask)):
        gz, gy, gx = image_gradient(im.to(torch.float64))
        norm = torch.sqrt(gz * gz + gy * gy + gx * gx)
        if mask is not None:
            w = (mask != 0).to(torch.float64).expand_as(norm)
            eps.append((norm * w).sum() / w.sum())
        else:
            eps.append(norm.mean())
    eps_f, eps_m = torch.stack(eps).tolist()
    return eps_f, eps_m


def ngf_forward(fixed, moving, eps_f, eps_m, upstream=None, want_map=True, want_coef=True, want_sums=True):
    """fixed (1 or C,1,D,H,W), moving (C,1,D,H,W), upstream u None (= 1) or (1 or C,1,D,H,W), float32 on the GPU; eps_f, eps_m
    finite and > 0 -> dict(d=(C,1,D,H,W) float32, coef=(C,3,D,H,W) float32 [c_z, c_y, c_x], sums=(C,) float64 [sum u d]); what is
    not wanted is None.  Two calls return the same bits, and chain c of a batch is the single-chain call."""
    if not torch.is_tensor(moving) or not torch.is_tensor(fixed):
        raise L.IrsError('fixed and moving must be tensors')
    Cn, D, H, W = _dims5(moving, 1)
    _chain_volumes('fixed', fixed, 'moving', Cn, D, H, W)
    eps_f, eps_m = _positive('eps_f', eps_f), _positive('eps_m', eps_m)
    if upstream is not None:
        _chain_volumes('upstream', upstream, 'moving', Cn, D, H, W)
    dev = moving.device
    d = torch.empty((Cn, 1, D, H, W), device=dev, dtype=torch.float32) if want_map else None
    coef = torch.empty((Cn, 3, D, H, W), device=dev, dtype=torch.float32) if want_coef else None
    sums = torch.empty(Cn, device=dev, dtype=torch.float64) if want_sums else None
    scratch = torch.empty(L.load().irs_reduce_scratch_doubles(), device=dev, dtype=torch.float64) if want_sums else None
    _call('irs_ngf_fwd', L.dev_ptr(fixed.contiguous(), torch.float32), fixed.shape[0], L.dev_ptr(moving.contiguous(), torch.float32),
          L.dev_ptr(None if upstream is None else upstream.contiguous(), torch.float32, allow_none=True),
          1 if upstream is None else upstream.shape[0], eps_f, eps_m, L.dev_ptr(d, None, True), L.dev_ptr(coef, None, True),
          L.dev_ptr(sums, None, True), L.dev_ptr(scratch, None, True), Cn, D, H, W)
    return {'d': d, 'coef': coef, 'sums': sums}


def ngf_backward(coef):
    """d(sum u d)/d(moving) (C,1,D,H,W) float32 = grad^T of the coefficient maps `coef` (C,3,D,H,W) of `ngf_forward`; it needs
    neither image"""
    if not torch.is_tensor(coef) or coef.dim() != 5 or coef.shape[1] != 3:
        raise L.IrsError(f'coef must have shape (C, 3, D, H, W), got {tuple(getattr(coef, "shape", ()))}')
    Cn, _, D, H, W = coef.shape
    g = torch.empty((Cn, 1, D, H, W), device=coef.device, dtype=torch.float32)
    _call('irs_ngf_bwd', L.dev_ptr(coef.contiguous(), torch.float32), L.dev_ptr(g), Cn, D, H, W)
    return g


def ngf_loss(fixed, moving, eps_f, eps_m, upstream=None):
    """(sum u d per chain (C,) float64, its gradient with respect to moving (C,1,D,H,W) float32)"""
    out = ngf_forward(fixed, moving, eps_f, eps_m, upstream, want_map=False)
    return out['sums'], ngf_backward(out['coef'])
