"""Coarse-to-fine chain start: the operators that carry an image pair down to a coarser grid and a velocity field up to a finer
one, and the `trainer.coarse_start` option.

The velocity field is stored in normalised coordinates (a displacement of 2 spans n - 1 voxels), so a field found on a coarse
grid means the same on a fine one and is prolonged without rescaling; every grid is align_corners, as every resize of
native.py.  `restrict_image` is a tent filter normalised per axis (full weighting at N = 2 n - 1), `restrict_mask` takes the
nearest fine voxel, `prolong_field` is trilinear: one HIP launch each (include/irsgmcmc.h: irs_restrict_image,
irs_restrict_mask, irs_prolong_field).  The trainer runs short chains on the restricted pair, level by level, and starts the
full-grid chains from the prolonged result (Trainer._coarse_start).

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import numbers

import torch

from . import _lib as L
from .ops import _call

MAX_LEVELS = 4
MIN_EXTENT = 9  # the smallest extent the engine is exercised at
LEVEL_KEYS = ('dims', 'no_iters', 'lr')


def _extents(name, dims):
    dims = tuple(dims.tolist() if hasattr(dims, 'tolist') else dims)
    if len(dims) != 3 or any(isinstance(n, bool) or not isinstance(n, numbers.Integral) for n in dims):
        raise L.IrsError(f'{name} must be three integers (d, h, w), got {dims!r}')
    return tuple(int(n) for n in dims)


def _volumes(name, t, ch=None):
    if t.dim() != 5 or (ch is not None and t.shape[1] != ch):
        raise L.IrsError(f'{name} must have shape (C,{ch if ch else "ch"},D,H,W), got {tuple(t.shape)}')
    return tuple(t.shape)


def restrict_image(im, dims):
    """im (Cim,1,D,H,W) float32 -> (Cim,1,d,h,w) with dims = (d, h, w), 2 <= d <= D and so on: the tent filter of
    include/irsgmcmc.h (irs_restrict_image).  Equal extents give the input back bit for bit.  No host synchronisation."""
    Cim, _, D, H, W = _volumes('im', im, 1)
    d, h, w = _extents('dims', dims)
    out = torch.empty((Cim, 1, d, h, w), device=im.device, dtype=torch.float32)
    _call('irs_restrict_image', L.dev_ptr(im, torch.float32), Cim, D, H, W, L.dev_ptr(out), d, h, w)
    return out


def restrict_mask(mask, dims):
    """mask (Cm,1,D,H,W) bool / uint8 -> (Cm,1,d,h,w) of the same dtype: every coarse voxel takes the nearest fine voxel
    (irs_restrict_mask).  No host synchronisation."""
    Cm, _, D, H, W = _volumes('mask', mask, 1)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise L.IrsError(f'mask must be bool or uint8, got {mask.dtype}')
    d, h, w = _extents('dims', dims)
    out = torch.empty((Cm, 1, d, h, w), device=mask.device, dtype=torch.uint8)
    src = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    _call('irs_restrict_mask', L.dev_ptr(src, torch.uint8), Cm, D, H, W, L.dev_ptr(out), d, h, w)
    return out.view(torch.bool) if mask.dtype == torch.bool else out


def prolong_field(x, dims):
    """x (C,ch,d,h,w) float32 -> (C,ch,D,H,W) with dims = (D, H, W), D >= d >= 2 and so on: trilinear, values not rescaled
    (irs_prolong_field).  ch is free: 3 for a velocity, 1 for a scalar volume.  No host synchronisation."""
    Cn, ch, d, h, w = _volumes('x', x)
    D, H, W = _extents('dims', dims)
    out = torch.empty((Cn, ch, D, H, W), device=x.device, dtype=torch.float32)
    _call('irs_prolong_field', L.dev_ptr(x, torch.float32), Cn, ch, d, h, w, L.dev_ptr(out), D, H, W)
    return out


def restrict_pair(fixed, moving, dims):
    """the pair a TransitionEngine takes, on the grid `dims`: fixed {'im', 'mask'} and moving {'im'} of (1 or C,1,D,H,W) ->
    ({'im', 'mask'}, {'im'}) of (.,1,d,h,w).  Always from the volumes given -- restrict from the full grid, not from a level."""
    return ({'im': restrict_image(fixed['im'], dims), 'mask': restrict_mask(fixed['mask'], dims)},
            {'im': restrict_image(moving['im'], dims)})


def _level(what, i, level):
    where = f'{what}.levels[{i}]'
    if not isinstance(level, dict):
        raise ValueError(f'{where} must be {{"dims": [d, h, w], "no_iters": n, "lr": optional}}, got {level!r}')
    unknown = set(level) - set(LEVEL_KEYS)
    if unknown:
        raise ValueError(f'{where}: unknown keys {sorted(unknown)}; known: {list(LEVEL_KEYS)}')
    for key in ('dims', 'no_iters'):
        if key not in level:
            raise ValueError(f'{where}: "{key}" is missing')
    dims = level['dims']
    if (not isinstance(dims, (list, tuple)) or len(dims) != 3 or
            any(isinstance(n, bool) or not isinstance(n, numbers.Integral) for n in dims)):
        raise ValueError(f'{where}.dims must be three integers [d, h, w], got {dims!r}')
    n = level['no_iters']
    if isinstance(n, bool) or not isinstance(n, numbers.Integral):
        raise ValueError(f'{where}.no_iters must be an integer, got {n!r}')
    if n < 1:
        raise ValueError(f'{where}: no_iters must be >= 1, got {n}')
    lr = level.get('lr')
    if lr is not None:
        if isinstance(lr, bool) or not isinstance(lr, numbers.Real) or not lr > 0 or lr == float('inf'):
            raise ValueError(f'{where}.lr must be a finite number > 0, got {lr!r}')
        lr = float(lr)
    return {'dims': tuple(int(x) for x in dims), 'no_iters': int(n), 'lr': lr}


def coarse_start_options(cfg_trainer, fine_dims, transformation_type):
    """`trainer.MCMC_init: "coarse"` with `trainer.coarse_start = {"levels": [{"dims": [d, h, w], "no_iters": n, "lr":
    optional}, ...]}`, the levels listed coarse to fine -> None when neither is there, else {'levels': [{'dims': (d, h, w),
    'no_iters': n, 'lr': float or None (the run's)}, ...]}.  Refuses one without the other, unknown keys, no level or more
    than MAX_LEVELS, an extent below MIN_EXTENT, a level larger than the next one or than the full grid on some axis, a last
    level that is the full grid, no_iters < 1, lr <= 0, SVFFD_3D (B-spline coefficients are not samples of the field) and a VI
    stage in the same run."""
    what = 'trainer.coarse_start'
    opt, init = cfg_trainer.get('coarse_start'), cfg_trainer.get('MCMC_init')
    if opt is None:
        if init == 'coarse':
            raise ValueError(f'trainer.MCMC_init = "coarse" needs {what} = {{"levels": [...]}}')
        return None
    if init != 'coarse':
        raise ValueError(f'{what} is set but trainer.MCMC_init = {init!r}; it takes effect with MCMC_init = "coarse" only')
    if not isinstance(opt, dict):
        raise ValueError(f'{what} must be {{"levels": [{{"dims": [d, h, w], "no_iters": n, "lr": optional}}, ...]}}, got {opt!r}')
    unknown = set(opt) - {'levels'}
    if unknown:
        raise ValueError(f"{what}: unknown keys {sorted(unknown)}; known: ['levels']")
    if transformation_type == 'SVFFD_3D':
        raise ValueError(f'{what}: SVFFD_3D is not supported (B-spline coefficients are not samples of the velocity field)')
    if cfg_trainer.get('VI'):
        raise ValueError(f'{what}: trainer.VI must be false (a coarse start replaces the VI stage as the source of the start)')
    levels = opt.get('levels')
    if not isinstance(levels, (list, tuple)) or not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f'{what}.levels must be a list of 1 .. {MAX_LEVELS} levels, got {levels!r}')
    levels = [_level(what, i, level) for i, level in enumerate(levels)]
    fine = tuple(int(n) for n in fine_dims)
    for i, level in enumerate(levels):
        dims = level['dims']
        if min(dims) < MIN_EXTENT:
            raise ValueError(f'{what}.levels[{i}]: dims {list(dims)} have an extent below {MIN_EXTENT}')
        above, name = (levels[i + 1]['dims'], f'levels[{i + 1}]') if i + 1 < len(levels) else (fine, 'the full grid')
        if any(a > b for a, b in zip(dims, above)):
            raise ValueError(f'{what}.levels[{i}]: dims {list(dims)} exceed {list(above)} of {name}')
    if levels[-1]['dims'] == fine:
        raise ValueError(f'{what}.levels[{len(levels) - 1}]: dims {list(fine)} are the full grid; the last level must be coarser')
    return {'levels': levels}
