"""numpy restatement of the cubic B-spline output resampling (include/irsgmcmc.h, "Cubic B-spline output resampling"), written
from the header's words: it shares no code with ir_sgmcmc_amd/bspline.py or the HIP path.  numpy rounds every operation once
and fuses none, so an expression formed in the documented order is the device's bit for bit.

Prefilter: float64 arithmetic, the line at rest in `store` (float32 as the device keeps it; float64 gives the recursion with
no storage rounding at all, the one that is compared with scipy).  Evaluation: in `dtype`, float32 as the device or float64
for the error bands.  The native rule stands on the helpers of tests/_native_resolution.py.
"""
import numpy as np
import torch

from tests import _native_resolution as R

Z1 = np.sqrt(3.0) - 2.0
_Z1Z1 = Z1 * Z1
ANTI = Z1 / (_Z1Z1 - 1.0)  # z1 / (z1^2 - 1)
SERIES = 32


def mirror(k, n):
    """whole-sample mirror of the index array k into [0, n - 1], applied once"""
    k = np.asarray(k)
    return np.where(k < 0, -k, np.where(k > n - 1, 2 * (n - 1) - k, k))


def prefilter_axis(s, axis, store=np.float32):
    """the lines of `s` along `axis` -> their coefficients, in `store`"""
    s = np.moveaxis(np.asarray(s), axis, 0).astype(np.float64)
    n = s.shape[0]
    assert n >= 2
    T = 2 * n - 2
    zk, acc = 1.0, np.zeros(s.shape[1:])
    for k in range(min(T, SERIES)):
        acc = acc + zk * (6.0 * s[k if k <= n - 1 else 2 * (n - 1) - k])
        zk = zk * Z1
    if T <= SERIES:
        acc = acc / (1.0 - zk)
    plus = np.empty(s.shape, store)  # c+ as it rests between the two sweeps
    run = acc
    plus[0] = run
    for k in range(1, n):
        run = 6.0 * s[k] + Z1 * run
        plus[k] = run
    rest = plus.astype(np.float64)
    c = np.empty(s.shape, store)
    run = ANTI * (rest[n - 1] + Z1 * rest[n - 2])
    c[n - 1] = run
    for k in range(n - 2, -1, -1):
        run = Z1 * (run - rest[k])
        c[k] = run
    return np.moveaxis(c, 0, axis)


def prefilter(im, store=np.float32):
    """im (..., D, H, W) -> coefficients in `store`: x (the last axis), then y, then z"""
    c = np.asarray(im)
    for axis in (-1, -2, -3):
        c = prefilter_axis(c, axis, store)
    return c


def _axis(q, n, dtype):
    """taps (4 index arrays) and weights (4 arrays in `dtype`) of one axis at the positions q"""
    f = dtype
    q = np.minimum(np.maximum(np.asarray(q, f), f(0)), f(n - 1))
    i0 = np.minimum(np.floor(q).astype(np.int64), n - 2)
    t = q - i0.astype(f)
    u = f(1) - t
    taps = [mirror(i0 - 1 + j, n) for j in range(4)]
    w = [u * u * u / f(6), (f(3) * t * t * t - f(6) * t * t + f(4)) / f(6), (f(3) * u * u * u - f(6) * u * u + f(4)) / f(6),
         t * t * t / f(6)]
    return taps, w


def evaluate(coeff, q, dtype=np.float32):
    """the spline of coeff (D,H,W) at q = (q_z, q_y, q_x), arrays of one shape in index coordinates -> values in `dtype`"""
    c = np.asarray(coeff).astype(dtype)
    D, H, W = c.shape
    (kz, wz), (ky, wy), (kx, wx) = _axis(q[0], D, dtype), _axis(q[1], H, dtype), _axis(q[2], W, dtype)
    vz = np.zeros(np.shape(q[0]), dtype)
    for a in range(4):
        vy = np.zeros_like(vz)
        for b in range(4):
            vx = np.zeros_like(vz)
            for j in range(4):
                vx = vx + wx[j] * c[kz[a], ky[b], kx[j]]
            vy = vy + wy[b] * vx
        vz = vz + wz[a] * vy
    return vz


def index_coordinates(transformation, dtype=np.float32):
    """transformation (3,D,H,W) in [-1,1], component 0 = x -> (q_z, q_y, q_x): ((g + 1) * 0.5) * (n - 1) in `dtype`"""
    g = np.asarray(transformation).astype(dtype)
    n = g.shape[1:]
    return tuple(((g[2 - a] + dtype(1)) * dtype(0.5)) * dtype(n[a] - 1) for a in range(3))


def warp(coeff, transformation, dtype=np.float32):
    """coeff (Cim,1,D,H,W), transformation (C,3,D,H,W) -> (C,1,D,H,W) in `dtype`"""
    coeff, transformation = np.asarray(coeff), np.asarray(transformation)
    out = [evaluate(coeff[c if coeff.shape[0] > 1 else 0, 0], index_coordinates(transformation[c], dtype), dtype)
           for c in range(transformation.shape[0])]
    return np.stack(out)[:, None]


# ---------------------------------------------------------------- the native rule
def native_float64(u, grid, im, coeff, fill):
    """u (C,3,*dims) float32 torch, im / coeff (Cim,1,*shape) float32 torch -> dict of numpy arrays (C,*shape): 'value' float64 (the
    spline of `coeff` at r - p where all eight trilinear taps of r lie in the native box, the trilinear blend with `fill`
    elsewhere), 'cubic' bool (which of the two), 'near_face' bool (r within 1e-3 of a face of the box, p_a or p_a + n_a - 1, on
    a padded axis: the class hangs on the last bits there)"""
    C = u.shape[0]
    r = R.source_coordinate(u, grid).numpy()  # (C,3,*shape), entry a = axis a, before the border clamp
    p, n, P = grid.padding, grid.shape, grid.padded
    cubic = np.ones(r.shape[:1] + r.shape[2:], bool)
    near = np.zeros_like(cubic)
    q = []
    for a in range(3):
        ra = np.minimum(np.maximum(r[:, a], 0.0), P[a] - 1.0)
        i0 = np.minimum(np.floor(ra).astype(np.int64), P[a] - 1)
        i1 = np.minimum(i0 + 1, P[a] - 1)
        cubic &= (i0 >= p[a]) & (i1 <= p[a] + n[a] - 1)
        if p[a] > 0:  # an unpadded axis has no face inside the padded box: the border clamp decides there, the same way in any precision
            near |= (np.abs(ra - p[a]) < 1e-3) | (np.abs(ra - (p[a] + n[a] - 1)) < 1e-3)
        q.append(ra - p[a])
    linear = R.native_warp(u, grid, torch.float64, im=im, fill=fill)['im'][:, 0].numpy()
    value = np.empty(cubic.shape)
    for c in range(C):
        spline = evaluate(coeff[c if coeff.shape[0] > 1 else 0, 0].numpy(), tuple(qa[c] for qa in q), np.float64)
        value[c] = np.where(cubic[c], spline, linear[c])
    return {'value': value, 'cubic': cubic, 'near_face': near}


def _tap32(r, last):
    f = np.floor(r)
    i0 = np.minimum(f.astype(np.int64), last)
    i1 = np.minimum(i0 + 1, last)
    return i0, i1, (f + np.float32(1)) - r, r - f  # i0, i1, w0, w1


def native_float32(u, grid, coeff):
    """the device's float32 path of the cubic voxels, operation by operation: the displacement interpolated at the grid
    coordinate (x, then y, then z), r = (i + p) + u (P - 1) / 2, the clamp, the class, the spline at r - p.
    -> ('value' float32 (C,*shape), meaningful where 'cubic' is set; 'cubic' bool)"""
    f = np.float32
    u = u.numpy().astype(f)
    C = u.shape[0]
    p, n, P, m = grid.padding, grid.shape, grid.padded, grid.dims
    idx = np.meshgrid(*[np.arange(k) for k in n], indexing='ij')
    taps = []
    for a in range(3):
        step = f(np.float64(m[a] - 1) / np.float64(P[a] - 1))
        g = np.minimum((idx[a] + p[a]).astype(f) * step, f(m[a] - 1))
        taps.append(_tap32(g, m[a] - 1))
    (z0, z1, wz0, wz1), (y0, y1, wy0, wy1), (x0, x1, wx0, wx1) = taps
    value = np.zeros((C, *n), f)
    cubic = np.ones((C, *n), bool)
    for c in range(C):
        uc = []
        for ch in range(3):
            fld = u[c, ch]
            pz = []
            for zz in (z0, z1):
                py = [wx0 * fld[zz, yy, x0] + wx1 * fld[zz, yy, x1] for yy in (y0, y1)]
                pz.append(wy0 * py[0] + wy1 * py[1])
            uc.append(wz0 * pz[0] + wz1 * pz[1])
        q = []
        for a in range(3):
            half = f(0.5) * f(P[a] - 1)
            raw = (idx[a] + p[a]).astype(f) + uc[2 - a] * half
            r = np.minimum(np.maximum(raw, f(0)), f(P[a] - 1))
            i0, i1, _, _ = _tap32(r, P[a] - 1)
            cubic[c] &= (i0 >= p[a]) & (i1 <= p[a] + n[a] - 1)
            q.append(r - f(p[a]))
        value[c] = evaluate(coeff[c if coeff.shape[0] > 1 else 0, 0].numpy(), tuple(q), f)
    return {'value': value, 'cubic': cubic}


# the cases of the native tests: (native shape, registration dims); the last one is a cube, which the data set does not pad
NATIVE_CASES = [((7, 12, 20), (9, 10, 11)), ((13, 9, 70), (9, 9, 12)), ((6, 33, 16), (10, 12, 9)), ((10, 10, 10), (9, 9, 9))]
NATIVE_SEEDS = (1, 2)


def native_inputs(shape, dims, seed, C=2):
    """(grid, u (C,3,*dims), im (1,1,*shape), fill) of one native case"""
    from ir_sgmcmc_amd.native import NativeGrid
    grid = NativeGrid.from_shape(shape, dims)
    im, _, _ = R.random_volumes(shape, seed)
    return grid, R.smooth_field(C, dims, seed), im, float(im.min())
