"""CPU restatement of the Hausdorff and percentile surface distances, for the tests: contours from
shifted comparisons, nearest squared distances by chunked brute force in float64, the order statistic by the index rule.
No code shared with the HIP path.  Also the label maps the surface-distance tests fuzz with."""
import functools
import math

import numpy as np

STRUCTURES = {'left_thalamus': 10, 'left_caudate': 11, 'left_putamen': 12, 'left_pallidum': 13, 'brain_stem': 16,
              'left_hippocampus': 17, 'left_amygdala': 18, 'left_accumbens': 26, 'right_thalamus': 49, 'right_caudate': 50,
              'right_putamen': 51, 'right_pallidum': 52, 'right_hippocampus': 53, 'right_amygdala': 54, 'right_accumbens': 58}
LABELS = list(STRUCTURES.values())


def contour(mask):
    """voxels of `mask` with a face neighbour inside the volume that is not in `mask`"""
    out = np.zeros_like(mask)
    for ax in range(3):
        for sh in (1, -1):
            nb = np.roll(mask, sh, axis=ax)
            valid = np.ones_like(mask)
            edge = [slice(None)] * 3
            edge[ax] = 0 if sh == 1 else -1
            valid[tuple(edge)] = False
            out |= mask & valid & ~nb
    return out


def nearest_d2(a, b, spacing):
    """squared distance (float64, spacing units; spacing = (sx, sy, sz), sx on the last axis) of every voxel of the boolean
    map `a` to the nearest voxel of `b`, in the order of np.argwhere(a)"""
    s_zyx = np.array([spacing[2], spacing[1], spacing[0]], dtype=np.float64)
    pa = np.argwhere(a).astype(np.float64) * s_zyx
    pb = np.argwhere(b).astype(np.float64) * s_zyx
    out = np.empty(len(pa))
    step = max(1, 4_000_000 // max(len(pb), 1))
    for i in range(0, len(pa), step):
        out[i:i + step] = ((pa[i:i + step, None, :] - pb[None, :, :]) ** 2).sum(-1).min(axis=1)
    return out


def order_index(q, n):
    """0-based index of the directed percentile q of n ascending distances"""
    return min(max(int(math.ceil(q * float(n) / 100.0)) - 1, 0), n - 1)


def directed_percentile(d2, q):
    """the order statistic of the squared distances d2 at percentile q (still squared)"""
    return np.sort(d2)[order_index(q, len(d2))]


def reference(seg_fixed, seg_moving, labels, spacing, percentiles):
    """seg_* numpy (Cf|C, 1, D, H, W) -> dict of float64 arrays of SQUARED distances in spacing units, exact in float64 for
    dyadic spacings: 'hd2' (C, L, 2) and 'pct2' (Q, C, L, 2) ([..., 0]: over the fixed contour, of the distance to the moving
    one), and 'asd' (C, L); inf where a contour is empty"""
    C, L, Q = seg_moving.shape[0], len(labels), len(percentiles)
    hd2 = np.full((C, L, 2), np.inf)
    pct2 = np.full((Q, C, L, 2), np.inf)
    asd = np.full((C, L), np.inf)
    for c in range(C):
        f = seg_fixed[c if seg_fixed.shape[0] > 1 else 0, 0]
        m = seg_moving[c, 0]
        for j, lab in enumerate(labels):
            a, b = contour(f == lab), contour(m == lab)
            if not a.any() or not b.any():
                continue
            means = []
            for direction, (src, dst) in enumerate(((a, b), (b, a))):
                d2 = nearest_d2(src, dst, spacing)
                hd2[c, j, direction] = d2.max()
                for i, q in enumerate(percentiles):
                    pct2[i, c, j, direction] = directed_percentile(d2, q)
                means.append(np.sqrt(d2).mean())
            asd[c, j] = 0.5 * (means[0] + means[1])
    return {'hd2': hd2, 'pct2': pct2, 'asd': asd}


# ------------------------------------------------------------------------------------------------ the fuzz generator
def random_seg(rng, dims, labels, touch_border=True):
    D, H, W = dims
    seg = np.zeros(dims, np.int16)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    for lab in labels:
        for _ in range(rng.integers(1, 3)):
            c = rng.uniform(0, 1, 3) * np.array(dims)
            r = rng.uniform(1.0, 0.25 * min(dims), 3)
            blob = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 < 1.0
            blob &= rng.uniform(size=dims) < 0.995  # holes make inner contours
            seg[blob] = lab
    if touch_border:
        seg[:, 0, :3] = labels[0]
    return seg


def fuzz_case(rng, dims, C, Cf):
    present = [l for l in LABELS if rng.uniform() < 0.8]
    f = np.stack([random_seg(rng, dims, present)[None] for _ in range(Cf)])
    m = np.stack([random_seg(rng, dims, [l for l in present if rng.uniform() < 0.9])[None] for _ in range(C)])
    # a single voxel, and a label whose box is the whole volume
    m[0, 0, dims[0] // 2, dims[1] // 2, dims[2] // 2] = 26
    f[0, 0, dims[0] // 3, dims[1] // 3, dims[2] // 3] = 26
    for s in (f, m):
        s[:, 0, 0, 0, 0] = 58
        s[:, 0, -1, -1, -1] = 58
        s[:, 0, dims[0] // 2:, :2, :] = 58
    return f, m


@functools.lru_cache(maxsize=None)
def fuzz_maps(dims, C, Cf):
    """the label maps of one fuzz case: the same for every test that asks"""
    rng = np.random.default_rng([7, C, Cf, *dims])
    f, m = fuzz_case(rng, dims, C, Cf)
    f.setflags(write=False)
    m.setflags(write=False)
    return f, m


@functools.lru_cache(maxsize=None)
def fuzz_reference(dims, C, Cf, spacing, percentiles):
    """reference() of fuzz_maps(dims, C, Cf), computed once and left unchanged"""
    f, m = fuzz_maps(dims, C, Cf)
    ref = reference(f, m, LABELS, spacing, percentiles)
    for v in ref.values():
        v.setflags(write=False)
    return ref
