"""Image posterior: volumes that live on the moving image's grid carried through every recorded transformation.

A recorded sample of the chain is a transformation; what a registration exists to move is an image.  The operators here fold,
per voxel of the fixed grid, the trilinear sample of S volumes under every recorded transformation into a Welford mean / M2, a
minimum and a maximum (include/irsgmcmc.h: irs_image_posterior_update -- one fused launch per step, no warped intermediate), and
turn one volume's state into the std, range and z maps and their masked summary (irs_image_posterior_finalize).  The sample is
bit for bit what `ops.warp` gives.

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import math
import os

import numpy as np
import torch

from . import _lib as L
from .ops import _call, _check_state, _dims5, _summary_buffers, _volume_mask

STATE_KEYS = ('mean', 'm2', 'low', 'high')
MAX_VOLUMES = L.IRS_IMAGE_POSTERIOR_MAX_VOLUMES
INT_COLUMNS = ('voxels', 'nonfinite_voxels', 'z_gt2', 'z_gt3')
FLOAT_COLUMNS = ('mean_sum', 'std_sum', 'std_max', 'range_max', 'z2_sum', 'z_max')


def image_posterior_state(S, dims, device):
    """the state of S volumes on a (D,H,W) grid: {'mean', 'm2', 'low', 'high'}, each (S,D,H,W) float32 zeros on `device`, 16 S
    bytes per voxel whatever the number of records.  The first update (records_before = 0) overwrites it."""
    dims = tuple(int(d) for d in dims)
    if isinstance(S, bool) or not isinstance(S, int) or not 1 <= S <= MAX_VOLUMES:
        raise L.IrsError(f'S must be an integer in 1 .. {MAX_VOLUMES}, got {S!r}')
    if len(dims) != 3 or min(dims) < 2:
        raise L.IrsError(f'dims must be three extents of at least 2, got {dims}')
    return {key: torch.zeros((S, *dims), device=device, dtype=torch.float32) for key in STATE_KEYS}


def _state_rows(state, shape):
    missing = [key for key in STATE_KEYS if key not in state]
    if missing:
        raise L.IrsError(f'state must hold {list(STATE_KEYS)}; {missing} missing')
    return tuple((key, state[key], shape, torch.float32) for key in STATE_KEYS)


def image_posterior_update(volumes, transformation, state, records_before):
    """Fold one recorded step into the image posterior: volumes (S,1,D,H,W) float32 on the moving image's grid, shared by the
    chains, S in 1 .. 8; transformation (C,3,D,H,W) float32 in [-1,1] coordinates, every chain's sample, as `ops.warp` takes it;
    state: the dict of image_posterior_state, updated in place with the C records in chain order after `records_before`
    records (0 overwrites it).  No host synchronisation."""
    Cn, D, H, W = _dims5(transformation, 3)
    if volumes.dim() != 5 or volumes.shape[1] != 1 or tuple(volumes.shape[2:]) != (D, H, W):
        raise L.IrsError(f'volumes shape {tuple(volumes.shape)} does not match transformation {tuple(transformation.shape)}: '
                         f'(S,1,{D},{H},{W}) expected')
    S = volumes.shape[0]
    if not 1 <= S <= MAX_VOLUMES:
        raise L.IrsError(f'{S} volumes: 1 .. {MAX_VOLUMES} are carried in one call')
    _check_state(*_state_rows(state, (S, D, H, W)))
    _call('irs_image_posterior_update', L.dev_ptr(volumes, torch.float32), S, L.dev_ptr(transformation, torch.float32), Cn, D, H, W,
          *(L.dev_ptr(state[key], torch.float32) for key in STATE_KEYS), int(records_before))


def image_posterior_finalize(state, index, n, reference=None, std_floor=0.0, mask=None):
    """The maps and the masked summary of volume `index` of the state after n records.  reference: a float32 volume of D H W
    elements on the fixed grid, or None; std_floor: finite and >= 0; mask (D,H,W) bool / uint8 or None.  -> (std, range,
    z | None, all (D,H,W) float32, isummary (4,) int64 INT_COLUMNS, fsummary (6,) float64 FLOAT_COLUMNS), on the device:
    std = sqrt(m2 / max(n - 1, 1)), range = high - low, z = (reference - mean) / sqrt(std^2 + std_floor^2); NaN where the mean
    is not finite.  include/irsgmcmc.h gives the columns.  No host synchronisation."""
    mean = state['mean'] if 'mean' in state else None
    if mean is None or mean.dim() != 4:
        raise L.IrsError(f'state must hold (S,D,H,W) tensors {list(STATE_KEYS)}')
    S, D, H, W = mean.shape
    _check_state(*_state_rows(state, (S, D, H, W)))
    if isinstance(index, bool) or not isinstance(index, int) or not 0 <= index < S:
        raise L.IrsError(f'index must be an integer in 0 .. {S - 1}, got {index!r}')
    std_floor = float(std_floor)
    if not (math.isfinite(std_floor) and std_floor >= 0):
        raise L.IrsError(f'std_floor must be finite and >= 0, got {std_floor}')
    dev = mean.device
    if reference is not None:
        if reference.numel() != D * H * W or reference.dtype != torch.float32:
            raise L.IrsError(f'reference must be a float32 ({D},{H},{W}) volume, got {reference.dtype} {tuple(reference.shape)}')
        reference = reference.reshape(D, H, W).contiguous()
    mask = _volume_mask(mask, D, H, W)
    ws, isummary, fsummary = _summary_buffers(L.IRS_IMAGE_POSTERIOR_WS_BYTES, L.IRS_IMAGE_POSTERIOR_SUMMARY_INTS,
                                              L.IRS_IMAGE_POSTERIOR_SUMMARY_FLOATS, dev)
    std, rng = (torch.empty((D, H, W), device=dev, dtype=torch.float32) for _ in range(2))
    z = torch.empty((D, H, W), device=dev, dtype=torch.float32) if reference is not None else None
    _call('irs_image_posterior_finalize', *(L.dev_ptr(state[key][index], torch.float32) for key in STATE_KEYS), D, H, W, int(n),
          L.dev_ptr(reference, torch.float32, True), std_floor, L.dev_ptr(mask, torch.uint8, True), L.dev_ptr(std), L.dev_ptr(rng),
          L.dev_ptr(z, None, True), L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws), L.IRS_IMAGE_POSTERIOR_WS_BYTES)
    return std, rng, z, isummary, fsummary


def load_volume(path, data_loader):
    """A NIfTI file on the registration grid, the way the loader puts the moving image there -> (1,1,D,H,W) float32 on the host,
    intensities as they are.  A loader over a BiobankDataset pads and resizes it as its images (the data set's _get_image:
    padding with the minimum to a cube, trilinear resize to dims); any other loader (the synthetic pair) takes an array of exactly
    its dims."""
    from .utils.imageio import read_nifti
    if not os.path.isfile(str(path)):
        raise FileNotFoundError(f'{path}: no such file')
    dataset = getattr(data_loader, 'dataset', None)
    if dataset is not None and hasattr(dataset, '_get_image'):
        return dataset._get_image(str(path)).unsqueeze(0).float().contiguous()
    dims = tuple(int(d) for d in data_loader.dims)
    arr, _ = read_nifti(str(path), np.float32)
    if tuple(arr.shape) != dims:
        raise ValueError(f'{path}: the volume has shape {tuple(arr.shape)}, the registration grid {dims}; without image files the '
                         f'loader ({type(data_loader).__name__}) resamples nothing')
    return torch.from_numpy(np.ascontiguousarray(arr)).reshape(1, 1, *dims)
