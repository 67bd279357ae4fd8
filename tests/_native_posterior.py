"""numpy restatement of the native-grid posteriors (csrc/native_posterior_kernels.hip on the steps of csrc/native_device.h), shared by
tests/test_native_posterior_host.py and tests/test_gpu_native_posterior.py.

`sample_np` restates, operation by operation in float32, what one chain's displacement makes of a native voxel: the trilinear
interpolation of the three channels at the voxel's grid coordinate, the source position in the padded frame, the nearest label
(half to even, 0 outside the native box) and the trilinear blend of the unpadded image with the fill.  `native_posterior_np` folds
the samples of a list of steps as the kernel does: counts += 1, the per-record volumes Welford-folded in float64 in record
order, the image through tests/_image_posterior.welford32.  `composition` is the yardstick of the GPU tests: the same state from
operators that exist without the fused kernel."""
import numpy as np

from tests._image_posterior import welford32

F32 = np.float32


def _tap(r, last):
    """native_tap: (i0, i1 int64, w0, w1 float32) of the position r in [0, last]"""
    f = np.floor(r).astype(F32)
    i0 = np.minimum(f.astype(np.int64), last)
    return i0, np.minimum(i0 + 1, last), ((f + F32(1.0)) - r).astype(F32), (r - f).astype(F32)


def _box(k, p, n):
    """box_index: the padded index k as (index clamped into the native box, whether it was in it)"""
    i = k - p
    return np.clip(i, 0, n - 1), (i >= 0) & (i < n)


def sample_np(u, grid, seg=None, im=None, fill=0.0):
    """u (3,*dims) float32 of ONE chain, seg int16 / im float32 (*shape) or None -> (label (*shape) int16 | None, intensity
    (*shape) float32 | None)"""
    n, p, P, m = grid.shape, grid.padding, grid.padded, grid.dims
    u = np.asarray(u, F32)
    idx = np.meshgrid(*[np.arange(k) for k in n], indexing='ij')
    ft = []
    for a in range(3):
        step = F32(float(m[a] - 1) / float(P[a] - 1))
        g = np.minimum(((idx[a] + p[a]).astype(F32) * step).astype(F32), F32(m[a] - 1))
        ft.append(_tap(g, m[a] - 1))
    uc = []
    for c in range(3):
        f = u[c]
        pz = []
        for zi in (ft[0][0], ft[0][1]):
            py = []
            for yi in (ft[1][0], ft[1][1]):
                py.append(((ft[2][2] * f[zi, yi, ft[2][0]]).astype(F32) + (ft[2][3] * f[zi, yi, ft[2][1]]).astype(F32)).astype(F32))
            pz.append(((ft[1][2] * py[0]).astype(F32) + (ft[1][3] * py[1]).astype(F32)).astype(F32))
        uc.append(((ft[0][2] * pz[0]).astype(F32) + (ft[0][3] * pz[1]).astype(F32)).astype(F32))
    r = []
    for a in range(3):
        half = F32(0.5) * F32(P[a] - 1)
        raw = ((idx[a] + p[a]).astype(F32) + (uc[2 - a] * half).astype(F32)).astype(F32)
        raw = np.where(np.isnan(raw), F32(0.0), raw)  # fmaxf drops a NaN
        r.append(np.minimum(np.maximum(raw, F32(0.0)), F32(P[a] - 1)).astype(F32))
    label = value = None
    if seg is not None:
        at, inside = [], np.ones(n, bool)
        for a in range(3):
            i, ok = _box(np.rint(r[a]).astype(np.int64), p[a], n[a])  # half to even
            at.append(i)
            inside &= ok
        label = np.where(inside, np.asarray(seg)[at[0], at[1], at[2]], 0).astype(np.int16)
    if im is not None:
        im = np.asarray(im, F32)
        taps = []
        for a in range(3):
            i0, i1, w0, w1 = _tap(r[a], P[a] - 1)
            taps.append(((_box(i0, p[a], n[a]), w0), (_box(i1, p[a], n[a]), w1)))
        value = np.zeros(n, F32)
        for (zi, zin), wz in taps[0]:
            for (yi, yin), wy in taps[1]:
                for (xi, xin), wx in taps[2]:
                    val = np.where(zin & yin & xin, im[zi, yi, xi], F32(fill)).astype(F32)
                    w = ((wx * wy).astype(F32) * wz).astype(F32)
                    value = (value + (val * w).astype(F32)).astype(F32)
    return label, value


def native_posterior_np(steps, grid, seg=None, labels=None, im=None, fill=0.0):
    """steps: a list of (C,3,*dims) float32 displacements; seg int16 / im float32 (Cim,*shape) with Cim 1 or C, or None.
    -> dict with 'counts' (K,*shape) int64, 'vol' (records, K) int64, 'vol_mean' / 'vol_m2' (K,) float64, 'mean', 'm2', 'low',
    'high' (*shape) float32 and 'records'"""
    records_l, records_x = [], []
    for u in steps:
        for c in range(u.shape[0]):
            pick = lambda vol: None if vol is None else vol[c if vol.shape[0] > 1 else 0]
            label, value = sample_np(u[c], grid, pick(seg), pick(im), fill)
            records_l.append(label)
            records_x.append(value)
    out = {'records': len(records_l)}
    if seg is not None:
        lab = np.asarray(labels).reshape(-1, 1, 1, 1)
        hit = np.stack(records_l)[:, None] == lab[None]            # (records, K, *shape)
        out['counts'] = hit.sum(axis=0).astype(np.int64)
        out['vol'] = hit.reshape(hit.shape[0], hit.shape[1], -1).sum(axis=2).astype(np.int64)
        mean, m2 = np.zeros(len(labels)), np.zeros(len(labels))
        for k, x in enumerate(out['vol'].astype(np.float64), 1):   # Welford in record order, as the device folds it
            d = x - mean
            mean = mean + d / k
            m2 = m2 + d * (x - mean)
        out['vol_mean'], out['vol_m2'] = mean, m2
    if im is not None:
        out['mean'], out['m2'], out['low'], out['high'] = welford32(records_x)
    return out
