"""Native-grid posteriors: the posterior label maps and the image posterior on the image's own voxel grid.

Every other posterior map lives on the registration grid `dims`; what a user opens in a viewer is on the voxel grid of the
image.  The operator here carries every chain's sampled displacement of one recorded step to the native grid and folds, per native
voxel, the nearest-neighbour label into the counts of the K structures and the trilinear sample of the native moving image into
a Welford mean / M2, a minimum and a maximum -- in ONE launch that forms no warped volume (include/irsgmcmc.h:
irs_native_posterior_update).  The label and the sample are bit for bit what `ops.native_warp` writes; the states are what
`ops.label_posterior_finalize` and `image_posterior.image_posterior_finalize` take, on the native extents.  The sample is always
trilinear, whatever trainer.output_interpolation says of the images that are saved.

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import ctypes as C
import logging
import math

import torch

from . import _lib as L
from . import image_posterior as _ip
from . import ops
from .ops import _call, _chain_volumes, _check_state, _dims5, _labels, _workspace

LABEL_KEYS = ('counts', 'volume')  # on the device; 'labels', the K label values, stays on the host
IMAGE_KEYS = _ip.STATE_KEYS


def state_bytes(grid, K=0, image=False):
    """bytes of the state on the device: 4 K + 16 (image) bytes per native voxel, and the 16 K bytes of the volume moments"""
    voxels = int(grid.shape[0]) * int(grid.shape[1]) * int(grid.shape[2])
    return (4 * K + (16 if image else 0)) * voxels + 16 * K


def native_posterior_state(grid, labels=None, image=False, device='cuda:0'):
    """The zeroed state on the native grid of `grid` (a native.NativeGrid): with `labels` (the K label values) 'counts'
    (K,*shape) int32 and 'volume' (K,2) float64 on `device` and 'labels' (K,) int32, the label values, on the host; with `image`
    'mean', 'm2', 'low', 'high' (*shape) float32 -- 4 K + 16 bytes per native voxel whatever the number of records (state_bytes,
    logged at debug level).  The first update (records_before = 0) overwrites the image part."""
    shape = tuple(int(n) for n in grid.shape)
    if len(shape) != 3 or min(shape) < 2:
        raise L.IrsError(f'the native shape must have three extents of at least 2, got {shape}')
    if labels is None and not image:
        raise L.IrsError('native_posterior_state: neither labels nor image asked for')
    state = {}
    if labels is not None:
        _, K = _labels(labels)
        if not 1 <= K <= L.IRS_MAX_LABELS:
            raise L.IrsError(f'1 .. {L.IRS_MAX_LABELS} labels, got {K}')
        state['counts'] = torch.zeros((K, *shape), device=device, dtype=torch.int32)
        state['volume'] = torch.zeros((K, 2), device=device, dtype=torch.float64)
        state['labels'] = torch.tensor([int(x) for x in labels], dtype=torch.int32)
    if image:
        state.update({key: torch.zeros(shape, device=device, dtype=torch.float32) for key in IMAGE_KEYS})
    logging.getLogger('default').debug(f'native posterior state: {state_bytes(grid, len(state.get("counts", ())), image)} bytes')
    return state


def _group(state, keys, what):
    have = [key for key in keys if key in state]
    if have and len(have) != len(keys):
        raise L.IrsError(f'the {what} part of the state must hold {list(keys)}; only {have} given')
    return bool(have)


def native_posterior_update(displacement, grid, state, records_before, seg=None, im=None, fill=None):
    """Fold one recorded step into the native-grid posteriors.  displacement (C,3,*grid.dims) float32 in [-1,1] coordinates, as
    `ops.native_warp` takes it; grid: a native.NativeGrid; state: the dict of native_posterior_state, updated in place with the C
    records in chain order after `records_before` records.  seg int16 (counted under the state's 'labels') and / or im float32:
    the UNPADDED native moving volumes, (1 or C,1,*grid.shape) with one leading size for both; each goes with its part of the
    state, and at least one must be given.  fill: what the data set padded the image with (default: the
    minimum of `im`, one host read-back).  No host synchronisation when `fill` is given."""
    Cn, D, H, W = _dims5(displacement, 3)
    if (D, H, W) != tuple(grid.dims):
        raise L.IrsError(f'displacement {tuple(displacement.shape)} is not on the registration grid {tuple(grid.dims)}')
    n = tuple(int(x) for x in grid.shape)
    with_labels, with_image = _group(state, LABEL_KEYS + ('labels',), 'label'), _group(state, IMAGE_KEYS, 'image')
    if with_labels != (seg is not None):
        raise L.IrsError('seg and the counts / volume / labels of the state go together: '
                         f'seg {"given" if seg is not None else "None"}, state {"with" if with_labels else "without"} them')
    if with_image != (im is not None):
        raise L.IrsError(f'im and the mean / m2 / low / high of the state go together: im {"given" if im is not None else "None"}, '
                         f'state {"with" if with_image else "without"} them')
    given = [(k, t, dt) for k, t, dt in (('im', im, torch.float32), ('seg', seg, torch.int16)) if t is not None]
    if not given:
        raise L.IrsError('native_posterior_update: neither seg nor im given')
    for k, t, dt in given:
        _chain_volumes(k, t, 'the native grid', Cn, *n)
        if t.dtype != dt:
            raise L.IrsError(f'{k} must be {dt}, got {t.dtype}')
        if t.shape[0] != given[0][1].shape[0]:
            raise L.IrsError(f'the moving volumes must share their leading size: {given[0][0]} has {given[0][1].shape[0]}, '
                             f'{k} has {t.shape[0]}')
    lab, K = (None, 0)
    if with_labels:
        lab, K = _labels(state['labels'].tolist())
        _check_state(('counts', state['counts'], (K, *n), torch.int32), ('volume', state['volume'], (K, 2), torch.float64))
    if with_image:
        _check_state(*((key, state[key], n, torch.float32) for key in IMAGE_KEYS))
        if fill is None:
            fill = float(im.min())
    fill = 0.0 if fill is None else float(fill)
    if not math.isfinite(fill):
        raise L.IrsError(f'fill must be finite, got {fill}')
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    ws, nbytes = _workspace('irs_native_posterior_workspace', Cn, K, i3(n), device=displacement.device)
    _call('irs_native_posterior_update', L.dev_ptr(displacement, torch.float32), Cn, i3(grid.dims), i3(n), i3(grid.padding),
          L.dev_ptr(im, None, True), L.dev_ptr(seg, None, True), given[0][1].shape[0], fill, lab, K,
          *(L.dev_ptr(state.get(key), None, True) for key in LABEL_KEYS), *(L.dev_ptr(state.get(key), None, True) for key in IMAGE_KEYS),
          int(records_before), L.dev_ptr(ws), nbytes)


def native_label_finalize(state, n, seg_fixed, mask=None):
    """`ops.label_posterior_finalize` on the native extents: seg_fixed, the NATIVE fixed segmentation of grid.shape elements
    (int16), mask the native fixed mask or None -> (entropy float32, map_label int16, summary int64, mask_summary float64)"""
    return ops.label_posterior_finalize(state['counts'], n, state['labels'].tolist(), seg_fixed, mask)


def native_image_finalize(state, n, reference=None, std_floor=0.0, mask=None):
    """`image_posterior.image_posterior_finalize` on the native extents: reference, the NATIVE fixed image (float32) or None,
    mask the native fixed mask or None -> (std, range, z | None, isummary, fsummary)"""
    return _ip.image_posterior_finalize({key: state[key].unsqueeze(0) for key in IMAGE_KEYS}, 0, n, reference, std_floor, mask)
