"""The three multi-resolution operators restated in numpy float64, from their definitions in include/irsgmcmc.h and sharing no
code with the HIP path: per axis a dense matrix of weights, the volume contracted with the three of them.

Along one axis coarse index i of n sits at fine coordinate x_i = i (N - 1) / (n - 1), fine index I of N at coarse coordinate
I (n - 1) / (N - 1).
"""
import math

import numpy as np


def fine_coordinate(i, N, n):
    return np.float64(i * (N - 1)) / np.float64(n - 1)


def restriction_matrix(N, n):
    """(n, N) float64: row i holds the tent of half-width r = max(1, (N - 1) / (n - 1)) around x_i -- every integer k with
    |k - x_i| < r weighs 1 - |k - x_i| / r on the fine voxel clamp(k, 0, N - 1) -- each weight divided by the sum of the row's"""
    assert 2 <= n <= N
    r = max(1.0, (N - 1) / (n - 1))
    M = np.zeros((n, N), np.float64)
    for i in range(n):
        x = fine_coordinate(i, N, n)
        taps = [(k, 1.0 - abs(k - x) / r) for k in range(math.floor(x - r) - 2, math.ceil(x + r) + 3) if abs(k - x) < r]
        total = 0.0
        for _, w in taps:
            total += w
        for k, w in taps:
            M[i, min(max(k, 0), N - 1)] += w / total
    return M


def prolongation_matrix(n, N):
    """(N, n) float64: row I holds the two linear weights at the coarse coordinate of fine index I; a tap at index n has weight 0
    and no entry"""
    assert 2 <= n <= N
    M = np.zeros((N, n), np.float64)
    for I in range(N):
        c = np.float64(I * (n - 1)) / np.float64(N - 1)
        i0 = min(math.floor(c), n - 1)
        f = c - i0
        M[I, i0] += 1.0 - f
        if i0 + 1 < n:
            M[I, i0 + 1] += f
        else:
            assert f == 0.0
    return M


def _contract(x, mats):
    """x (..., A, B, C) with mats of shapes (a, A), (b, B), (c, C) -> (..., a, b, c), in float64"""
    return np.einsum('ai,bj,ck,...ijk->...abc', *mats, np.asarray(x, np.float64), optimize=False)


def restrict_image(im, dims):
    """im (..., D, H, W) -> float64 (..., d, h, w)"""
    return _contract(im, [restriction_matrix(N, n) for N, n in zip(im.shape[-3:], dims)])


def prolong_field(x, dims):
    """x (..., d, h, w) -> float64 (..., D, H, W)"""
    return _contract(x, [prolongation_matrix(n, N) for n, N in zip(x.shape[-3:], dims)])


def nearest_index(N, n):
    """(n,) int: floor(x_i + 0.5)"""
    return np.array([min(math.floor(fine_coordinate(i, N, n) + 0.5), N - 1) for i in range(n)], np.int64)


def restrict_mask(mask, dims):
    """mask (..., D, H, W) -> (..., d, h, w) of the same dtype: the fine voxel at floor(x_i + 0.5) per axis"""
    iz, iy, ix = (nearest_index(N, n) for N, n in zip(mask.shape[-3:], dims))
    return mask[..., iz[:, None, None], iy[None, :, None], ix[None, None, :]]
