"""A numpy restatement of every operator of ir_sgmcmc_amd/masks.py, written from the definitions in include/irsgmcmc.h and
sharing no code with the HIP path: components by a plain breadth-first flood fill (no scipy), morphology by a brute-force
minimum over the offsets of the ball.  tests/test_masks_host.py holds it against scipy.ndimage; the GPU tests then need only
this file.  Everything takes and returns (D,H,W) arrays of ONE volume."""
import itertools
from collections import deque

import numpy as np


def neighbour_offsets(connectivity):
    """the offsets (dz, dy, dx) in {-1, 0, 1}^3 with 1 .. k non-zero components, k = 1, 2, 3 for connectivity 6, 18, 26"""
    k = {6: 1, 18: 2, 26: 3}[connectivity]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(c != 0 for c in o) <= k]


def connected_components(mask, connectivity=26):
    """-> (labels int32, n): flood fill from every unlabelled set voxel in ascending linear order, so a component's number is the
    rank of its smallest linear index"""
    mask = np.asarray(mask) != 0
    D, H, W = mask.shape
    offsets = neighbour_offsets(connectivity)
    labels = np.zeros(mask.shape, np.int32)
    n = 0
    for start in zip(*np.nonzero(mask)):  # np.nonzero lists in C (linear) order
        if labels[start]:
            continue
        n += 1
        labels[start] = n
        queue = deque([start])
        while queue:
            z, y, x = queue.popleft()
            for dz, dy, dx in offsets:
                p = (z + dz, y + dy, x + dx)
                if 0 <= p[0] < D and 0 <= p[1] < H and 0 <= p[2] < W and mask[p] and not labels[p]:
                    labels[p] = n
                    queue.append(p)
    return labels, n


def canonical_labels(labels):
    """any labelling (0 background) renumbered 1 .. n by first occurrence in linear order"""
    flat = np.asarray(labels).reshape(-1)
    values, first = np.unique(flat[flat != 0], return_index=True)
    order = values[np.argsort(first)]
    lut = np.zeros(int(flat.max()) + 1 if flat.size else 1, np.int32)
    lut[order] = np.arange(1, order.size + 1, dtype=np.int32)
    return lut[flat].reshape(np.asarray(labels).shape).astype(np.int32)


def keep_largest(mask, connectivity=26, keep=1):
    labels, n = connected_components(mask, connectivity)
    sizes = np.bincount(labels.reshape(-1), minlength=n + 1)[1:]
    order = sorted(range(n), key=lambda i: (-sizes[i], i))[:keep]  # ties: the smaller number
    return np.isin(labels, [i + 1 for i in order]) & (labels > 0)


def fill_holes(mask):
    """the mask plus the background components (6-connected) that have no voxel on the border of the volume"""
    mask = np.asarray(mask) != 0
    labels, n = connected_components(~mask, 6)
    border = np.zeros(mask.shape, bool)
    border[[0, -1], :, :] = border[:, [0, -1], :] = border[:, :, [0, -1]] = True
    open_labels = np.unique(labels[border & (labels > 0)])
    return mask | ((labels > 0) & ~np.isin(labels, open_labels))


def ball_r2(radius):
    return int(np.floor(float(radius) ** 2 + 1e-9))


def squared_distance(mask, r2):
    """min(r2 + 1, squared distance in voxels to the nearest set voxel): the minimum over every offset of the ball, brute force"""
    mask = np.asarray(mask) != 0
    D, H, W = mask.shape
    R = int(np.floor(np.sqrt(r2)))
    best = np.full(mask.shape, r2 + 1, np.int64)
    for dz, dy, dx in itertools.product(range(-R, R + 1), repeat=3):
        d2 = dz * dz + dy * dy + dx * dx
        if d2 > r2 or abs(dz) >= D or abs(dy) >= H or abs(dx) >= W:  # outside the ball, or past the volume from every voxel
            continue
        # out[z, y, x] sees mask[z + dz, y + dy, x + dx] where that lies inside the volume
        zs, ys, xs = (slice(max(0, -d), n - max(0, d)) for d, n in ((dz, D), (dy, H), (dx, W)))
        zt, yt, xt = (slice(max(0, d), n - max(0, -d)) for d, n in ((dz, D), (dy, H), (dx, W)))
        view = best[zs, ys, xs]
        np.minimum(view, np.where(mask[zt, yt, xt], d2, r2 + 1), out=view)
    return best


def dilate(mask, radius):
    r2 = ball_r2(radius)
    return np.asarray(mask) != 0 if r2 == 0 else squared_distance(mask, r2) <= r2


def erode(mask, radius):
    return ~dilate(~(np.asarray(mask) != 0), radius)


def close(mask, radius):
    return erode(dilate(mask, radius), radius)


def open(mask, radius):  # noqa: A001
    return dilate(erode(mask, radius), radius)


def intensity_histogram(im, bins, value_range, mask=None):
    """the bin rule of include/irsgmcmc.h in float32, every operation rounded once"""
    im = np.asarray(im, np.float32)
    lo, hi = np.float32(value_range[0]), np.float32(value_range[1])
    inv_w = np.float32(bins) / np.float32(hi - lo)
    take = np.isfinite(im) if mask is None else np.isfinite(im) & (np.asarray(mask) != 0)
    with np.errstate(invalid='ignore', over='ignore'):
        t = np.floor((im - lo).astype(np.float32) * inv_w).astype(np.float32)
    b = np.minimum(np.maximum(t, np.float32(0)), np.float32(bins - 1))
    return np.bincount(b[take].astype(np.int64), minlength=bins).astype(np.int64)


def otsu_threshold(counts, value_range):
    """the inner edge that maximises the between-class variance, a plain loop in float64; the first of equal maxima"""
    c = np.asarray(counts, np.float64).reshape(-1)
    lo, hi = float(value_range[0]), float(value_range[1])
    bins = c.size
    width = (hi - lo) / bins
    centres = [lo + (i + 0.5) * width for i in range(bins)]
    total = c.sum()
    best, best_k = -1.0, None
    for k in range(1, bins):
        n0, n1 = c[:k].sum(), c[k:].sum()
        v = 0.0
        if n0 > 0 and n1 > 0:
            mu0 = sum(c[i] * centres[i] for i in range(k)) / n0
            mu1 = sum(c[i] * centres[i] for i in range(k, bins)) / n1
            v = (n0 / total) * (n1 / total) * (mu0 - mu1) ** 2
        if v > best:
            best, best_k = v, k
    return lo + best_k * width


def foreground_mask(im, threshold, connectivity=26, keep=1, fill=True, closing=2, dilation=0):
    """the chain of masks.foreground_mask for a numeric threshold -> (mask, {stage: voxels})"""
    mask = np.asarray(im, np.float32) > np.float32(threshold)
    voxels = {'threshold': int(mask.sum())}
    mask = keep_largest(mask, connectivity, keep)
    voxels['keep_largest'] = int(mask.sum())
    if fill:
        mask = fill_holes(mask)
        voxels['fill_holes'] = int(mask.sum())
    if ball_r2(closing) > 0:
        mask = close(mask, closing)
        voxels['closing'] = int(mask.sum())
    if ball_r2(dilation) > 0:
        mask = dilate(mask, dilation)
        voxels['dilation'] = int(mask.sum())
    return mask, voxels
