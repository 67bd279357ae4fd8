"""Bending energy of a velocity field: the second-order differential operator (`utils.diff_op.HessianOperator`, the
reference's `GradientOperator` applied twice) as two HIP operators.

    y_c = sum over component, axis pair (a, b) and voxel of (d_a d_b v_comp)^2

with forward differences whose difference array is replicate-padded, in both applications.  `bending_energy` is what a
`RegLoss_*` with `diff_op='HessianOperator'` evaluates and what the fused transition logs as its regulariser energy;
`bending_energy_grad` is its exact gradient, `2 H^T W H v`, the stencil of the transition's update with that prior.
"""
import torch

from . import _lib as L
from .ops import _call, _dims5


def _field(v):
    if not torch.is_tensor(v) or v.dim() != 5 or v.shape[1] != 3 or min(v.shape[2:]) < 2:
        raise L.IrsError(f'expected a (C,3,D,H,W) velocity field with every dim >= 2, got {tuple(getattr(v, "shape", ()))}')
    if v.dtype != torch.float32:
        raise L.IrsError(f'expected torch.float32, got {v.dtype}')
    return v.contiguous()


def bending_energy(v):
    """y per chain of the (C,3,D,H,W) float32 field `v` on the GPU -> (C,) float64.  float32 differences, float64 sums in a
    fixed order: two calls return the same bits."""
    v = _field(v)
    Cn, D, H, W = _dims5(v, 3)
    y = torch.empty(Cn, device=v.device, dtype=torch.float64)
    scratch = torch.empty(L.load().irs_reduce_scratch_doubles(), device=v.device, dtype=torch.float64)
    _call('irs_bending_energy', L.dev_ptr(v, torch.float32), L.dev_ptr(y), L.dev_ptr(scratch), Cn, D, H, W)
    return y


def bending_energy_grad(v, scale=None):
    """scale_c * dy_c/dv -> (C,3,D,H,W) float32; `scale`: None (= 1), a number, or C values (one per chain)."""
    v = _field(v)
    Cn, D, H, W = _dims5(v, 3)
    if scale is not None:
        scale = torch.as_tensor(scale, dtype=torch.float32, device=v.device).reshape(-1)
        if scale.numel() == 1:
            scale = scale.expand(v.shape[0])
        if scale.numel() != v.shape[0]:
            raise L.IrsError(f'scale must hold one value per chain ({v.shape[0]}), got {scale.numel()}')
        scale = scale.contiguous()
    out = torch.empty(v.shape, device=v.device, dtype=torch.float32)
    _call('irs_bending_energy_grad', L.dev_ptr(v, torch.float32), L.dev_ptr(scale, torch.float32, allow_none=True), L.dev_ptr(out), Cn, D, H, W)
    return out
