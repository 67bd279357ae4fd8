"""Cubic B-spline resampling of the images the package writes, and the `trainer.output_interpolation` option.

The chain warps trilinearly, because its adjoint is the trilinear sampler's; the files people open and measure on need not be.
`prefilter` turns a volume into the coefficients of its interpolating cubic B-spline (whole-sample mirror boundaries),
`warp` evaluates that spline at a transformation on the registration grid -- the twin of ops.warp -- and `native_warp_cubic` is
the image output of ops.native_warp with the same rule inside the native box and the trilinear blend with the fill outside it.
include/irsgmcmc.h (irs_bspline_prefilter, irs_bspline_warp, irs_native_warp_cubic) has the definition, operation by operation.

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import ctypes as C
import math

import torch

from . import _lib as L
from .ops import _call, _chain_volumes, _dims5

INTERPOLATIONS = ('linear', 'cubic')


def _image(name, im):
    if im.dim() != 5 or im.shape[1] != 1 or im.dtype != torch.float32:
        raise L.IrsError(f'{name} must be a (Cim,1,D,H,W) float32 tensor, got {im.dtype} {tuple(im.shape)}')
    return tuple(im.shape)


def prefilter(im):
    """im (Cim,1,D,H,W) float32, every extent >= 2 -> the coefficients of its interpolating cubic B-spline, same shape
    (irs_bspline_prefilter).  No host synchronisation."""
    Cim, _, D, H, W = _image('im', im)
    coeff = torch.empty_like(im)
    _call('irs_bspline_prefilter', L.dev_ptr(im, torch.float32), L.dev_ptr(coeff), Cim, D, H, W)
    return coeff


def warp(coeff, transformation):
    """coeff (1 or C,1,D,H,W): prefilter() of the image; transformation (C,3,D,H,W) float32 in [-1,1] -> (C,1,D,H,W) float32,
    the spline at every voxel's transformed position (irs_bspline_warp; border clamp, as ops.warp).  No host synchronisation."""
    Cn, D, H, W = _dims5(transformation, 3)
    _image('coeff', coeff)
    _chain_volumes('coeff', coeff, 'transformation', Cn, D, H, W)
    out = torch.empty((Cn, 1, D, H, W), device=transformation.device, dtype=torch.float32)
    _call('irs_bspline_warp', L.dev_ptr(coeff, torch.float32), coeff.shape[0], L.dev_ptr(transformation, torch.float32),
          L.dev_ptr(out), Cn, D, H, W)
    return out


def native_warp_cubic(displacement, grid, im, coeff=None, fill=None):
    """The image of ops.native_warp with the cubic rule.  displacement (C,3,*grid.dims) float32 in [-1,1] coordinates; grid: a
    native.NativeGrid; im (1 or C,1,*grid.shape) float32: the UNPADDED native moving image; coeff: prefilter(im) (default:
    formed here); fill: what the data set padded the image with (default: the minimum of `im`, one host read-back).
    -> (C,1,*grid.shape) float32: the spline where all eight trilinear taps of the source position lie in the native box,
    ops.native_warp's value elsewhere (irs_native_warp_cubic).  No host synchronisation when `fill` is given."""
    Cn, D, H, W = _dims5(displacement, 3)
    if (D, H, W) != tuple(grid.dims):
        raise L.IrsError(f'displacement {tuple(displacement.shape)} is not on the registration grid {tuple(grid.dims)}')
    n = tuple(grid.shape)
    _image('im', im)
    _chain_volumes('im', im, 'the native grid', Cn, *n)
    if coeff is None:
        coeff = prefilter(im)
    elif tuple(coeff.shape) != tuple(im.shape):
        raise L.IrsError(f'coeff shape {tuple(coeff.shape)} does not match im {tuple(im.shape)}')
    fill = float(im.min()) if fill is None else float(fill)
    if not math.isfinite(fill):
        raise L.IrsError(f'fill must be finite, got {fill}')
    out = torch.empty((Cn, 1, *n), device=displacement.device, dtype=torch.float32)
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    _call('irs_native_warp_cubic', L.dev_ptr(displacement, torch.float32), Cn, i3(grid.dims), i3(n), i3(grid.padding),
          L.dev_ptr(im, torch.float32), L.dev_ptr(coeff, torch.float32), im.shape[0], fill, L.dev_ptr(out))
    return out


def output_interpolation_options(cfg_trainer):
    """`trainer.output_interpolation`: absent, null or "linear" -> None (every written image is the chain's trilinear one);
    "cubic" -> {'order': 3}.  Anything else is refused."""
    value = cfg_trainer.get('output_interpolation')
    if value is None or (isinstance(value, str) and value == 'linear'):
        return None
    if isinstance(value, str) and value == 'cubic':
        return {'order': 3}
    raise ValueError(f'trainer.output_interpolation must be "linear" or "cubic", got {value!r}')
