"""Automatic foreground masks: the operators that make a mask from an image -- intensity histogram and Otsu threshold, connected
components, the largest components, hole filling, morphology with a Euclidean ball -- their chain `foreground_mask`, and the
`trainer.auto_mask` option.

Every operator takes (C,1,D,H,W) volumes on the device and treats the C volumes independently; a mask is bool or uint8 and comes
back in the dtype it was given in.  The work is HIP (include/irsgmcmc.h: irs_intensity_histogram, irs_mask_threshold,
irs_connected_components, irs_mask_keep_largest, irs_mask_fill_holes, irs_mask_dilate); every result is a function of the input
alone, so two calls are bit-identical.  Only `otsu_threshold` (host, float64), `intensity_histogram` without a range and
`foreground_mask` synchronise with the host.

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import math
import numbers

import numpy as np
import torch

from . import _lib as L
from .ops import _as_uint8, _call, _workspace, intensity_ranges

CONNECTIVITIES = (6, 18, 26)
MAX_RADIUS = L.IRS_MASK_MAX_RADIUS
AUTO_MASK_KEYS = ('source', 'which', 'threshold', 'bins', 'connectivity', 'keep', 'fill_holes', 'closing', 'dilation', 'save')
AUTO_MASK_DEFAULTS = {'source': 'image', 'which': 'both', 'threshold': 'otsu', 'bins': 256, 'connectivity': 26, 'keep': 1,
                      'fill_holes': True, 'closing': 2, 'dilation': 1, 'save': True}


def _mask_volumes(name, mask):
    """the mask as contiguous uint8 and its (C, D, H, W)"""
    if mask.dim() != 5 or mask.shape[1] != 1:
        raise L.IrsError(f'{name} must have shape (C,1,D,H,W), got {tuple(mask.shape)}')
    if mask.dtype not in (torch.bool, torch.uint8):
        raise L.IrsError(f'{name} must be bool or uint8, got {mask.dtype}')
    return _as_uint8(mask), (mask.shape[0], mask.shape[2], mask.shape[3], mask.shape[4])


def _like(out, mask):
    return out.view(torch.bool) if mask.dtype == torch.bool else out


def _integer(name, value, lo, hi):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or not lo <= value <= hi:
        raise L.IrsError(f'{name} must be an integer in {lo} .. {hi}, got {value!r}')
    return int(value)


def _connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise L.IrsError(f'connectivity must be 6, 18 or 26, got {connectivity!r}')
    return int(connectivity)


def ball_r2(radius):
    """the squared radius the ball morphology compares against: floor(radius^2 + 1e-9), an integer; refuses a radius that is
    negative, not finite or above MAX_RADIUS"""
    if isinstance(radius, bool) or not isinstance(radius, numbers.Real) or not math.isfinite(radius) or radius < 0:
        raise L.IrsError(f'radius must be a finite number >= 0, got {radius!r}')
    if radius > MAX_RADIUS:
        raise L.IrsError(f'radius = {radius!r} voxels: the ball morphology takes radii up to {MAX_RADIUS}')
    return int(math.floor(float(radius) ** 2 + 1e-9))


# ---- histogram and threshold
def intensity_histogram(im, bins=256, value_range=None, mask=None):
    """im (C,1,D,H,W) float32 -> (C,bins) int64 on the device: exact counts of the finite values, under mask ((1 or C,1,D,H,W)
    bool / uint8) when there is one.  Bins over value_range = (lo, hi) by the rule of image_similarity (fp32; a value outside
    lands in the first or the last bin); None: ops.intensity_ranges of the whole of im, one host read-back."""
    if im.dim() != 5 or im.shape[1] != 1:
        raise L.IrsError(f'im must have shape (C,1,D,H,W), got {tuple(im.shape)}')
    Cn, _, D, H, W = im.shape
    bins = _integer('bins', bins, L.IRS_MASK_MIN_BINS, L.IRS_MASK_MAX_BINS)
    im_ptr = L.dev_ptr(im, torch.float32)
    m, Cm = None, 0
    if mask is not None:
        m, (Cm, *dims) = _mask_volumes('mask', mask)
        if tuple(dims) != (D, H, W) or Cm not in (1, Cn):
            raise L.IrsError(f'mask shape {tuple(mask.shape)} does not match im: (1 or {Cn},1,{D},{H},{W}) expected')
    lo, hi = intensity_ranges(im)[0] if value_range is None else (float(x) for x in value_range)
    hist = torch.empty((Cn, bins), device=im.device, dtype=torch.int64)
    _call('irs_intensity_histogram', im_ptr, Cn, L.dev_ptr(m, torch.uint8, True), Cm, D, H, W, lo, hi, bins, L.dev_ptr(hist))
    return hist


def otsu_threshold(counts, value_range):
    """The Otsu threshold of ONE histogram: counts (bins,) or (1,bins), integers (a tensor or an array), over value_range = (lo,
    hi).  On the host, in float64: among the inner bin edges lo + k (hi - lo) / bins, k = 1 .. bins - 1, the one that maximises
    the between-class variance w0 w1 (mu0 - mu1)^2 of the bins below and above it (bin centres as values); ties go to the lowest
    edge.  Raises for an empty histogram and for one with a single occupied bin (no edge separates anything)."""
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    c = c.reshape(-1) if c.ndim == 2 and c.shape[0] == 1 else c
    if c.ndim != 1 or c.size < 2:
        raise ValueError(f'otsu_threshold: counts must be one histogram of at least 2 bins, got shape {tuple(c.shape)}')
    if (c < 0).any():
        raise ValueError('otsu_threshold: negative counts')
    lo, hi = (float(x) for x in value_range)
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f'otsu_threshold: value_range ({lo}, {hi}), finite bounds with hi > lo needed')
    c = c.astype(np.float64)
    total = c.sum()
    if total == 0:
        raise ValueError('otsu_threshold: the histogram is empty')
    if np.count_nonzero(c) < 2:
        raise ValueError('otsu_threshold: the histogram has a single occupied bin: nothing to separate')
    bins = c.size
    width = (hi - lo) / bins
    centres = lo + (np.arange(bins, dtype=np.float64) + 0.5) * width
    n0 = np.cumsum(c)[:-1]            # counts below edge k = 1 .. bins - 1
    s0 = np.cumsum(c * centres)[:-1]
    n1, s1 = total - n0, (c * centres).sum() - s0
    ok = (n0 > 0) & (n1 > 0)
    between = np.zeros(bins - 1)
    between[ok] = (n0[ok] / total) * (n1[ok] / total) * (s0[ok] / n0[ok] - s1[ok] / n1[ok]) ** 2
    k = int(np.argmax(between)) + 1   # argmax takes the first of equal maxima: the lowest edge
    return lo + k * width


def threshold_mask(im, threshold):
    """im (C,1,D,H,W) float32 -> bool mask im > threshold (a NaN is background).  No host synchronisation."""
    if im.dim() != 5 or im.shape[1] != 1:
        raise L.IrsError(f'im must have shape (C,1,D,H,W), got {tuple(im.shape)}')
    Cn, _, D, H, W = im.shape
    out = torch.empty(tuple(im.shape), device=im.device, dtype=torch.uint8)
    _call('irs_mask_threshold', L.dev_ptr(im, torch.float32), Cn, D, H, W, float(threshold), L.dev_ptr(out))
    return out.view(torch.bool)


# ---- components
def connected_components(mask, connectivity=26):
    """mask (C,1,D,H,W) bool / uint8 -> (labels (C,1,D,H,W) int32, counts (C,) int32): background 0, the components of each volume
    numbered 1 .. n in ascending order of their smallest linear voxel index; connectivity 6, 18 or 26.  No host synchronisation."""
    m, (Cn, D, H, W) = _mask_volumes('mask', mask)
    connectivity = _connectivity(connectivity)
    m_ptr = L.dev_ptr(m, torch.uint8)
    ws, nbytes = _workspace('irs_connected_components_workspace', Cn, D, H, W, device=mask.device)
    labels = torch.empty(tuple(mask.shape), device=mask.device, dtype=torch.int32)
    counts = torch.empty(Cn, device=mask.device, dtype=torch.int32)
    _call('irs_connected_components', m_ptr, Cn, D, H, W, connectivity, L.dev_ptr(labels), L.dev_ptr(counts), L.dev_ptr(ws), nbytes)
    return labels, counts


def keep_largest(mask, connectivity=26, keep=1):
    """the `keep` largest components of every volume of mask (ties: the smaller component number, i.e. the one that starts first);
    fewer components than `keep`: all of them; an empty mask stays empty.  No host synchronisation."""
    m, (Cn, D, H, W) = _mask_volumes('mask', mask)
    connectivity = _connectivity(connectivity)
    keep = _integer('keep', keep, 1, L.IRS_MASK_MAX_KEEP)
    m_ptr = L.dev_ptr(m, torch.uint8)
    ws, nbytes = _workspace('irs_mask_select_workspace', Cn, D, H, W, device=mask.device)
    out = torch.empty(tuple(mask.shape), device=mask.device, dtype=torch.uint8)
    _call('irs_mask_keep_largest', m_ptr, Cn, D, H, W, connectivity, keep, L.dev_ptr(out), L.dev_ptr(ws), nbytes)
    return _like(out, mask)


def fill_holes(mask):
    """mask plus the background voxels with no 6-connected background path to the border of their volume
    (scipy.ndimage.binary_fill_holes with its default structure).  No host synchronisation."""
    m, (Cn, D, H, W) = _mask_volumes('mask', mask)
    m_ptr = L.dev_ptr(m, torch.uint8)
    ws, nbytes = _workspace('irs_mask_select_workspace', Cn, D, H, W, device=mask.device)
    out = torch.empty(tuple(mask.shape), device=mask.device, dtype=torch.uint8)
    _call('irs_mask_fill_holes', m_ptr, Cn, D, H, W, L.dev_ptr(out), L.dev_ptr(ws), nbytes)
    return _like(out, mask)


_fill_holes = fill_holes  # foreground_mask and margin_mask take a flag of that name


# ---- ball morphology
def _ball(mask, radius, erosions):
    """the dilations (False) and erosions (True) listed, one after the other, with the ball of `radius` voxels"""
    m, (Cn, D, H, W) = _mask_volumes('mask', mask)
    r2 = ball_r2(radius)
    L.dev_ptr(m, torch.uint8)
    if r2 == 0:  # the ball is the voxel itself
        return mask
    ws, nbytes = _workspace('irs_mask_morphology_workspace', Cn, D, H, W, device=mask.device)
    for erode in erosions:
        out = torch.empty(tuple(mask.shape), device=mask.device, dtype=torch.uint8)
        _call('irs_mask_dilate', L.dev_ptr(m, torch.uint8), Cn, D, H, W, r2, int(erode), L.dev_ptr(out), L.dev_ptr(ws), nbytes)
        m = out
    return _like(m, mask)


def dilate(mask, radius):
    """the voxels within `radius` voxels (Euclidean, compared as integers: squared distance <= ball_r2(radius)) of a set voxel.
    radius 0 returns the input; radii up to MAX_RADIUS.  No host synchronisation."""
    return _ball(mask, radius, (False,))


def erode(mask, radius):
    """~dilate(~mask): voxels outside the volume are not background, so a mask on the border is not eaten from there"""
    return _ball(mask, radius, (True,))


def close(mask, radius):
    """erode(dilate(mask))"""
    return _ball(mask, radius, (False, True))


def open(mask, radius):  # noqa: A001  (the operator's name, as scipy.ndimage and every morphology package has it)
    """dilate(erode(mask))"""
    return _ball(mask, radius, (True, False))


# ---- the pipeline
def bounding_box(mask):
    """mask (1,1,D,H,W) -> [[z0, z1], [y0, y1], [x0, x1]], half-open, of its set voxels (None when it is empty); synchronises"""
    m = mask.reshape(mask.shape[-3:]) != 0
    box = []
    for axis in range(3):
        hit = torch.nonzero(m.any(dim=tuple(a for a in range(3) if a != axis))).flatten()
        if hit.numel() == 0:
            return None
        box.append([int(hit[0]), int(hit[-1]) + 1])
    return box


def foreground_mask(im, threshold='otsu', bins=256, connectivity=26, keep=1, fill_holes=True, closing=2, dilation=0):  # noqa: A002
    """The foreground of ONE image im (1,1,D,H,W) float32 -> (mask (1,1,D,H,W) bool, summary): im > threshold (`'otsu'`: the Otsu
    threshold of its `bins`-bin histogram; a number: that number), the `keep` largest components, holes filled, a closing and a
    dilation with balls of `closing` / `dilation` voxels (0: the step is left out).  summary: {'threshold', 'components' (found
    after the threshold), 'voxels': {stage: count} in the order the stages ran, 'total' (voxels of the volume), 'bounding_box'}.
    Synchronises (it reads the histogram and the counts).  Raises a ValueError that names the stage after which the mask was
    empty or covered the whole volume."""
    if im.dim() != 5 or tuple(im.shape[:2]) != (1, 1):
        raise L.IrsError(f'im must have shape (1,1,D,H,W), got {tuple(im.shape)}')
    total = im[0, 0].numel()
    summary = {'voxels': {}, 'total': total}
    if isinstance(threshold, str):
        if threshold != 'otsu':
            raise ValueError(f"threshold must be 'otsu' or a number, got {threshold!r}")
        value_range = intensity_ranges(im)[0]
        threshold = otsu_threshold(intensity_histogram(im, bins, value_range), value_range)
    elif isinstance(threshold, bool) or not isinstance(threshold, numbers.Real) or not math.isfinite(threshold):
        raise ValueError(f"threshold must be 'otsu' or a finite number, got {threshold!r}")
    summary['threshold'] = float(threshold)

    def stage(name, m):
        n = int(m.sum())
        summary['voxels'][name] = n
        if n == 0 or n == total:
            raise ValueError(f'foreground_mask: the mask {"is empty" if n == 0 else "covers the whole volume"} after the stage '
                             f'"{name}" (threshold {summary["threshold"]:g}, {total} voxels)')
        return m

    mask = stage('threshold', threshold_mask(im, threshold))
    summary['components'] = int(connected_components(mask, connectivity)[1][0])
    mask = stage('keep_largest', keep_largest(mask, connectivity, keep))
    if fill_holes:
        mask = stage('fill_holes', _fill_holes(mask))
    if ball_r2(closing) > 0:
        mask = stage('closing', close(mask, closing))
    if ball_r2(dilation) > 0:
        mask = stage('dilation', dilate(mask, dilation))
    summary['bounding_box'] = bounding_box(mask)
    return mask, summary


def margin_mask(mask, fill_holes=True, closing=0, dilation=0):  # noqa: A002
    """the safety margin of a mask that came from a file: holes filled, a closing and a dilation, as in foreground_mask ->
    (mask, summary with 'voxels', 'total' and 'bounding_box')"""
    total = mask[0, 0].numel()
    summary = {'voxels': {'file': int(mask.sum())}, 'total': total}
    if fill_holes:
        mask = _fill_holes(mask)
        summary['voxels']['fill_holes'] = int(mask.sum())
    if ball_r2(closing) > 0:
        mask = close(mask, closing)
        summary['voxels']['closing'] = int(mask.sum())
    if ball_r2(dilation) > 0:
        mask = dilate(mask, dilation)
        summary['voxels']['dilation'] = int(mask.sum())
    summary['bounding_box'] = bounding_box(mask)
    return mask, summary


# ---- the option
def _radius_option(what, key, value):
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) or not 0 <= value <= MAX_RADIUS:
        raise ValueError(f'{what}.{key} must be a number in 0 .. {MAX_RADIUS} (voxels), got {value!r}')
    return float(value)


def auto_mask_options(cfg_trainer):
    """`trainer.auto_mask = {"source": "image" | "file", "which": "both" | "fixed" | "moving", "threshold": "otsu" | number, "bins",
    "connectivity", "keep", "fill_holes", "closing", "dilation", "save"}` -> None when the option is absent, else the dict with
    every key present (AUTO_MASK_DEFAULTS for the missing ones).  Unknown keys, wrong types and out-of-range values raise a
    ValueError that names the key.  With "source": "file" only fill_holes / closing / dilation act, on the masks read from files."""
    what = 'trainer.auto_mask'
    opt = cfg_trainer.get('auto_mask')
    if opt is None:
        return None
    if not isinstance(opt, dict):
        raise ValueError(f'{what} must be an object with the keys {list(AUTO_MASK_KEYS)}, got {opt!r}')
    unknown = set(opt) - set(AUTO_MASK_KEYS)
    if unknown:
        raise ValueError(f'{what}: unknown keys {sorted(unknown)}; known: {list(AUTO_MASK_KEYS)}')
    out = dict(AUTO_MASK_DEFAULTS)
    out.update(opt)
    if out['source'] not in ('image', 'file'):
        raise ValueError(f'{what}.source must be "image" or "file", got {out["source"]!r}')
    if out['which'] not in ('both', 'fixed', 'moving'):
        raise ValueError(f'{what}.which must be "both", "fixed" or "moving", got {out["which"]!r}')
    t = out['threshold']
    if isinstance(t, str):
        if t != 'otsu':
            raise ValueError(f'{what}.threshold must be "otsu" or a number, got {t!r}')
    elif isinstance(t, bool) or not isinstance(t, numbers.Real) or not math.isfinite(t):
        raise ValueError(f'{what}.threshold must be "otsu" or a finite number, got {t!r}')
    else:
        out['threshold'] = float(t)
    for key, lo, hi in (('bins', L.IRS_MASK_MIN_BINS, L.IRS_MASK_MAX_BINS), ('keep', 1, L.IRS_MASK_MAX_KEEP)):
        v = out[key]
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
            raise ValueError(f'{what}.{key} must be an integer in {lo} .. {hi}, got {v!r}')
        out[key] = int(v)
    if isinstance(out['connectivity'], bool) or out['connectivity'] not in CONNECTIVITIES:
        raise ValueError(f'{what}.connectivity must be 6, 18 or 26, got {out["connectivity"]!r}')
    for key in ('fill_holes', 'save'):
        if not isinstance(out[key], bool):
            raise ValueError(f'{what}.{key} must be true or false, got {out[key]!r}')
    for key in ('closing', 'dilation'):
        out[key] = _radius_option(what, key, out[key])
    return out


def auto_mask_sides(opt):
    return {'both': ('fixed', 'moving'), 'fixed': ('fixed',), 'moving': ('moving',)}[opt['which']]


def auto_mask(im, file_mask, opt):
    """one side of the option: im (1,1,D,H,W), file_mask (1,1,D,H,W) bool or None -> (mask bool, summary).  source "image":
    foreground_mask(im); "file": margin_mask(file_mask)."""
    if opt['source'] == 'image':
        return foreground_mask(im, opt['threshold'], opt['bins'], opt['connectivity'], opt['keep'], opt['fill_holes'], opt['closing'],
                               opt['dilation'])
    if file_mask is None:
        raise ValueError('trainer.auto_mask: "source": "file" needs a mask read from a file')
    return margin_mask(file_mask.bool(), opt['fill_holes'], opt['closing'], opt['dilation'])
