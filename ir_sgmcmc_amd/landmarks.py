"""Landmark files, their coordinates on the registration grid and the host half of the landmark summary (host only; absent in
the reference, which scores a registration by its segmentations alone).

A landmark file is plain text: one landmark per line, three numbers separated by blanks or commas, in the axis order of the
array as `read_nifti` returns it -- (i0, i1, i2) indexes the native volume the way the data set does; `#` starts a comment.
The operators take points in [-1,1] coordinates with component 0 = x, the LAST axis (ops.transform_points), so `grid_points`
and `registration_grid_points` reverse the order.  DESIGN.md section 6, "Landmark propagation and TRE", has the definitions.
"""
import math

import numpy as np


def read_points(path, index_base=0):
    """-> (K,3) float64 voxel indices counted from 0.  index_base: 0, or 1 for files that count voxels from 1.  Raises
    ValueError naming the file and the line for anything but three finite numbers, and for a file without a landmark."""
    if index_base not in (0, 1) or isinstance(index_base, bool):
        raise ValueError(f'read_points: index_base must be 0 or 1, got {index_base!r}')
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            text = line.split('#', 1)[0].strip()
            if not text:
                continue
            tokens = text.replace(',', ' ').split()
            try:
                values = [float(t) for t in tokens]
            except ValueError:
                values = None
            if values is None or len(values) != 3 or not all(math.isfinite(v) for v in values):
                raise ValueError(f'{path}, line {no}: three finite numbers separated by blanks or commas expected, got {line.rstrip()!r}')
            rows.append(values)
    if not rows:
        raise ValueError(f'{path}: no landmark found')
    return np.asarray(rows, dtype=np.float64) - float(index_base)


def _normalised(grid_coordinates, dims):
    """grid coordinates (K,3) in registration-grid voxels per axis (D,H,W) -> [-1,1] coordinates (K,3) in x, y, z order"""
    g = np.asarray(grid_coordinates, dtype=np.float64).reshape(-1, 3)
    nm1 = np.asarray([int(m) - 1 for m in dims], dtype=np.float64)
    if len(dims) != 3 or nm1.min() < 1:
        raise ValueError(f'three dims of at least 2 needed, got {tuple(dims)}')
    return np.ascontiguousarray((2.0 * g / nm1 - 1.0)[:, ::-1])


def grid_points(native_indices, grid):
    """native voxel indices (K,3) in the axis order of the native array -> [-1,1] coordinates (K,3) float64 of the registration
    grid in x, y, z component order (component 0 belongs to the LAST axis), through NativeGrid.grid_coordinate"""
    idx = np.asarray(native_indices, dtype=np.float64).reshape(-1, 3)
    return _normalised([grid.grid_coordinate(tuple(row)) for row in idx], grid.dims)


def registration_grid_points(voxel_indices, dims):
    """the same for loaders without native volumes: voxel indices (K,3) of the registration grid, in (D,H,W) order"""
    return _normalised(voxel_indices, dims)


def _pearson(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size < 2:
        return float('nan')
    da, db = a - a.mean(), b - b.mean()
    den = math.sqrt(float((da * da).sum()) * float((db * db).sum()))
    return float((da * db).sum()) / den if den > 0 else float('nan')


def landmark_summary(table, summary, levels):
    """The dict of DESIGN.md section 6 from the finalize's table and reduced columns (host numpy / ints / floats).
    table (K,10) float64 with the columns ops.LANDMARK_COLUMNS; summary = (isummary {landmarks, landmarks without a finite
    sample, landmarks with a finite pit}, fsummary {sum / max tre_of_mean, sum tre_mean, max tre_max}); levels: the coverage
    levels.  What needs a sort or a pairing is done here, in double: the median of tre_of_mean, coverage_{level} = the share
    of the finite pit values <= level (the nominal value is the level itself) and the Pearson correlation of tre_of_mean with
    the largest principal std over the landmarks where both are finite.  Entries are NaN where nothing enters them."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 10)
    (landmarks, empty, with_pit), (om_sum, om_max, sm_sum, s_max) = [int(x) for x in summary[0]], [float(x) for x in summary[1]]
    valid = landmarks - empty
    nan = float('nan')
    of_mean, major, pit = table[:, 4], table[:, 5], table[:, 9]
    seen = table[:, 0] > 0
    pits = pit[np.isfinite(pit)]
    both = seen & np.isfinite(of_mean) & np.isfinite(major)
    out = {'landmarks': landmarks, 'empty_landmarks': empty, 'landmarks_with_pit': with_pit,
           'of_mean_mean': om_sum / valid if valid else nan, 'of_mean_median': float(np.median(of_mean[seen])) if valid else nan,
           'of_mean_max': om_max if valid else nan, 'sample_mean': sm_sum / valid if valid else nan,
           'sample_max': s_max if valid else nan,
           'coverage': {f'{float(p):g}': float((pits <= float(p)).mean()) if pits.size else nan for p in levels},
           'error_spread_correlation': _pearson(of_mean[both], major[both])}
    return out
