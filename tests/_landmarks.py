"""numpy restatement of the landmark operators ("Landmark propagation and TRE"), the input recipes and
the tolerances, shared by the host and GPU tests.  Written from the definitions, not from the kernels.

`sample(points, field, dtype)` is the trilinear sampler of the definitions (border clamp, align_corners) with every operation
carried out in `dtype`, in the order the contract of irs_transform_points states: numpy rounds each float32 operation once and
fuses nothing, so dtype = float32 is the kernel's arithmetic and dtype = float64 the reference.

Bound on |sampled32 - sampled64| (`sample_bound`), u = 2^-24, inputs (points, field) float32 and therefore exact in both:

  position.  Per axis the index coordinate is raw = fl(fl(fl(g + 1) * 0.5) * (n - 1)).  The sum rounds once (relative u), the
    halving is exact, the product rounds once (relative u): raw = raw_exact (1 + d1)(1 + d2), |d| <= u, so |raw - raw_exact| <=
    2 u raw_exact to first order.  The clamp to [0, n - 1] is 1-Lipschitz and fixes both ends, so the clamped coordinate is
    off by at most 2 u (n - 1).  floor, i - floor(i) and (floor(i) + 1) - i are exact in float32 (differences of multiples of
    ulp(i) no larger than 1): the weights of the COMPUTED position are exact and sum to 1.
    The exact trilinear interpolant is continuous, and along an axis its slope inside a cell is a convex combination of the
    four edge differences of the cell: it is Lipschitz per axis with constant L, the largest difference of the field between
    face-adjacent voxels.  Moving the position by 2 u (n_a - 1) along each of the three axes moves the value by at most
        3 * 2 u (n_max - 1) L = 6 u (n_max - 1) L.
  value.  At the computed position the kernel forms, per corner, w = fl(fl(wx wy) wz) (two roundings), t = fl(val w) (one) and
    adds the eight terms in order starting from 0 (the first sum is exact, so a term passes through at most 7 rounded sums):
    at most 10 roundings per term, (1 + u)^10 - 1 = 10 u to first order, on terms whose exact sum of magnitudes is
    sum_j |val_j| w_j <= max |d| because the exact weights sum to 1:
        10 u max|d|.
  Together  |sampled32 - sampled64| <= SECOND_ORDER * u * (10 max|d| + 6 (n_max - 1) L),  a = 10, b = 6; SECOND_ORDER = 1.001
  covers the terms of order u^2 (at most 16 u relative to the first-order ones) and the float64 reference's own rounding
  (2^-29 relative to u).  `mapped = fl(fl(scale * sampled) + offset)` adds two roundings: `mapped_bound`.

The recorder (`update`, `finalize`) is restated in float64 with a two-pass covariance and numpy.linalg.eigvalsh.  Bounds of the
device's float64 Welford state against it for n records per landmark (`state_bounds`), v = 2^-53, X = max |x| over the
landmark's samples, R = max range of a component, following tests/_displacement_covariance.py:
  mean      each of the n Welford steps rounds a difference, a quotient and a sum of size <= X, and the two-pass mean n sums:
            Em = 4 n v X.
  comoment  M_ab = sum_k delta_a e_b; a term carries the errors of delta and e (Em each), three roundings of its own and at most
            n - 1 of the running sum, |delta|, |e| <= R:  dM = (n + 2) v n R^2 + 2 n Em R + n Em^2 for the device, the same
            again for the two-pass reference:  EM = 2 dM.
  tre       e = sqrt(sum (x - t)^2) carries 6 roundings, E_e = 6 v e_max; the Welford mean of e as above: Et = 4 n v e_max + E_e;
            tre_m2 as a co-moment with R = range of e: Em2.
  All multiplied by FACTOR = 2 for what the first-order count leaves out.
The table is held to what those give by perturbation theory (`table_bounds`): |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|,
|a - b| / sqrt(b)) for the roots; Weyl for the eigenvalues of S = M / (n - 1) with |dS|_F <= sqrt(6) EM / (n - 1) plus the
solver's off-diagonal remainder 1e-15 |S|_F; for m = r' S^-1 r, |dm| <= 2 |r| |dr| / l_min + |r|^2 E_S / (l_min (l_min - E_S));
for pit the largest density of chi-square(3), exp(-1/2) / sqrt(2 pi) < 0.2420, times |dm|, plus 8 v for erf / exp / sqrt.
"""
import math

import numpy as np

U = 2.0 ** -24
V64 = 2.0 ** -53
A_VALUE, B_POSITION, SECOND_ORDER = 10.0, 6.0, 1.001
FACTOR = 2.0
COLUMNS = ('count', 'tre_mean', 'tre_std', 'tre_max', 'tre_of_mean', 'std_major', 'std_middle', 'std_minor', 'mahalanobis2', 'pit')
CHI2_3_MAX_DENSITY = 0.2420


# ---------------------------------------------------------------- the sampler
def sample(points, field, dtype=np.float64):
    """points (K,3) float32 [-1,1] coordinates (x, y, z); field (C,3,D,H,W) float32 -> (C,K,3) in `dtype`: the three channels
    sampled trilinearly, border clamp, align_corners, every operation in `dtype`; NaN rows for non-finite points"""
    dtype = np.dtype(dtype).type
    pts = np.asarray(points, dtype=np.float32)
    f = np.asarray(field, dtype=np.float32).astype(dtype)
    C, _, D, H, W = f.shape
    ok = np.isfinite(pts).all(axis=1)
    g = np.where(ok[:, None], pts, np.float32(0)).astype(dtype)
    taps = []
    for c, n in enumerate((W, H, D)):
        nm1 = dtype(n - 1)
        raw = ((g[:, c] + dtype(1)) * dtype(0.5)) * nm1
        i = np.where(raw <= 0, dtype(0), np.where(raw >= nm1, nm1, raw)).astype(dtype)
        fl = np.floor(i)
        i0 = fl.astype(np.int64)
        taps.append((i0, np.minimum(i0 + 1, n - 1), ((fl + dtype(1)) - i).astype(dtype), (i - fl).astype(dtype)))
    (x0, x1, wx0, wx1), (y0, y1, wy0, wy1), (z0, z1, wz0, wz1) = taps
    acc = np.zeros((C, 3, len(pts)), dtype=dtype)
    for zi, wz in ((z0, wz0), (z1, wz1)):
        for yi, wy in ((y0, wy0), (y1, wy1)):
            for xi, wx in ((x0, wx0), (x1, wx1)):   # x fastest
                w = ((wx * wy).astype(dtype) * wz).astype(dtype)
                acc = (acc + (f[:, :, zi, yi, xi] * w).astype(dtype)).astype(dtype)
    out = np.ascontiguousarray(acc.transpose(0, 2, 1))
    out[:, ~ok] = np.nan
    assert out.dtype == dtype
    return out


def mapped(sampled, scale, offset, dtype=np.float64):
    """scale_c * sampled_c + offset_c in `dtype` (scale: three float32 values; offset (K,3) float32 or None = 0)"""
    dtype = np.dtype(dtype).type
    sc = np.asarray(scale, dtype=np.float32).astype(dtype)
    off = np.zeros(sampled.shape[1:], dtype=dtype) if offset is None else np.asarray(offset, dtype=np.float32).astype(dtype)
    return ((np.asarray(sampled, dtype=dtype) * sc).astype(dtype) + off).astype(dtype)


def adjacent_difference(field):
    """L: the largest difference of the field between face-adjacent voxels, over chains, channels and axes"""
    f = np.asarray(field, dtype=np.float64)
    return max(float(np.abs(np.diff(f, axis=a)).max()) for a in (2, 3, 4))


def sample_bound(field):
    """the bound of the module docstring on |sampled32 - sampled64|, one number for the whole field"""
    f = np.asarray(field, dtype=np.float64)
    n_max = max(f.shape[2:])
    return SECOND_ORDER * U * (A_VALUE * float(np.abs(f).max()) + B_POSITION * (n_max - 1) * adjacent_difference(f))


def mapped_bound(field, scale, offset, mapped64):
    """... on |mapped32 - mapped64|: the bound on sampled times the channel's scale, one rounding of the product and one of the
    sum (of sizes <= |scale| max|d| and <= max |mapped|) -> (3,) per channel"""
    sc = np.abs(np.asarray(scale, dtype=np.float64))
    big = float(np.abs(np.asarray(field, dtype=np.float64)).max())
    top = float(np.nanmax(np.abs(mapped64))) if np.isfinite(mapped64).any() else 0.0
    return SECOND_ORDER * (sc * sample_bound(field) + U * sc * big + U * top)


# ---------------------------------------------------------------- the recorder, float64
def chi2_cdf3(x):
    """F3(x) = erf(sqrt(x / 2)) - sqrt(2 x / pi) exp(-x / 2)"""
    return math.erf(math.sqrt(x / 2.0)) - math.sqrt(2.0 * x / math.pi) * math.exp(-x / 2.0)


def update(records, target):
    """records: a list of (C,K,3) float32 arrays in record order; target (K,3) float32 -> per landmark the list of its finite
    samples in order (chains within a step), float64 (n_k,3)"""
    target = np.asarray(target, dtype=np.float32).astype(np.float64)
    flat = np.concatenate([np.asarray(r, dtype=np.float32).astype(np.float64) for r in records], axis=0)   # (n,K,3)
    fin = np.isfinite(flat).all(axis=2) & np.isfinite(target).all(axis=1)[None]
    return [flat[fin[:, k], k] for k in range(flat.shape[1])]


def finalize(samples, target):
    """-> dict: table (K,10) float64 with the columns COLUMNS, mean (K,3), comoment (K,6: xx, xy, xz, yy, yz, zz), tre_m2 (K),
    S (K,3,3), isummary [landmarks, count == 0, finite pit], fsummary [sum / max tre_of_mean, sum tre_mean, max tre_max]"""
    target = np.asarray(target, dtype=np.float32).astype(np.float64)
    K = len(samples)
    table = np.full((K, 10), np.nan)
    mean, M, S, m2 = np.zeros((K, 3)), np.zeros((K, 6)), np.zeros((K, 3, 3)), np.zeros(K)
    for k, x in enumerate(samples):
        n = len(x)
        table[k, 0] = n
        if n == 0:
            continue
        mu = x.sum(axis=0) / n
        dev = x - mu
        cm = dev.T @ dev
        cov = cm / max(n - 1, 1)
        e = np.sqrt(((x - target[k]) ** 2).sum(axis=1))
        em = e.sum() / n
        m2[k] = ((e - em) ** 2).sum()
        lam = np.linalg.eigvalsh(cov)[::-1]
        r = mu - target[k]
        table[k, 1:8] = [em, math.sqrt(m2[k] / max(n - 1, 1)), e.max(), math.sqrt(float(r @ r)), *np.sqrt(np.maximum(lam, 0.0))]
        if n >= 4 and lam[2] > 0:
            table[k, 8] = float(r @ np.linalg.solve(cov, r))
            table[k, 9] = chi2_cdf3(table[k, 8])
        mean[k], S[k] = mu, cov
        M[k] = [cm[0, 0], cm[0, 1], cm[0, 2], cm[1, 1], cm[1, 2], cm[2, 2]]
    seen = table[:, 0] > 0
    isummary = [K, int((~seen).sum()), int(np.isfinite(table[:, 9]).sum())]
    fsummary = ([float(table[seen, 4].sum()), float(table[seen, 4].max()), float(table[seen, 1].sum()), float(table[seen, 3].max())]
                if seen.any() else [0.0, -math.inf, 0.0, -math.inf])
    return {'table': table, 'mean': mean, 'comoment': M, 'tre_m2': m2, 'S': S, 'isummary': isummary, 'fsummary': fsummary}


def state_bounds(samples, target):
    """the bounds of the module docstring per landmark -> dict of (K,) arrays: mean, comoment, tre_mean, tre_m2"""
    target = np.asarray(target, dtype=np.float32).astype(np.float64)
    K = len(samples)
    out = {k: np.zeros(K) for k in ('mean', 'comoment', 'tre_mean', 'tre_m2')}
    for k, x in enumerate(samples):
        n = len(x)
        if n == 0:
            continue
        X, R = float(np.abs(x).max()), float((x.max(axis=0) - x.min(axis=0)).max())
        e = np.sqrt(((x - target[k]) ** 2).sum(axis=1))
        e_max, Re = float(e.max()), float(e.max() - e.min())
        Em = 4 * n * V64 * X
        co = lambda Em_, R_: 2 * ((n + 2) * V64 * n * R_ * R_ + 2 * n * Em_ * R_ + n * Em_ * Em_)
        Ee = 6 * V64 * e_max
        Et = 4 * n * V64 * e_max + Ee
        out['mean'][k], out['comoment'][k] = FACTOR * Em, FACTOR * co(Em, R)
        out['tre_mean'][k], out['tre_m2'][k] = FACTOR * Et, FACTOR * co(Et, Re + 2 * Ee)
    return out


def _root_bound(err, ref):
    """|sqrt(a) - sqrt(ref)| given |a - ref| <= err, a, ref >= 0"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.minimum(np.sqrt(err), np.where(ref > 0, err / np.sqrt(np.where(ref > 0, ref, 1.0)), np.inf))


def table_bounds(ref, bounds):
    """-> (K,10) tolerances of the table against finalize()'s, from state_bounds() by the perturbation theory of the docstring
    (inf where the theory gives nothing: E_S >= l_min)"""
    t, S = ref['table'], ref['S']
    K = len(t)
    tol = np.zeros((K, 10))
    n = t[:, 0]
    inv = 1.0 / np.maximum(n - 1, 1)
    tol[:, 1] = bounds['tre_mean']
    tol[:, 2] = _root_bound(bounds['tre_m2'] * inv, ref['tre_m2'] * inv)
    tol[:, 3] = bounds['tre_mean']          # the largest e: E_e is inside Et
    tol[:, 4] = math.sqrt(3.0) * bounds['mean'] + 8 * V64 * np.nan_to_num(t[:, 4])
    normS = np.sqrt((S ** 2).sum(axis=(1, 2)))
    ES = math.sqrt(6.0) * bounds['comoment'] * inv + 1e-15 * normS
    lam = np.nan_to_num(t[:, 5:8]) ** 2
    for j in range(3):
        tol[:, 5 + j] = _root_bound(ES, lam[:, j]) + 4 * V64 * np.nan_to_num(t[:, 5 + j])
    r, dr, lmin = np.nan_to_num(t[:, 4]), math.sqrt(3.0) * bounds['mean'], lam[:, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        dm = np.where(lmin > 2 * ES, 2 * r * dr / lmin + r * r * ES / (lmin * (lmin - ES)), np.inf)
        dm = dm + 16 * V64 * np.nan_to_num(t[:, 8])
    tol[:, 8] = FACTOR * dm
    tol[:, 9] = CHI2_3_MAX_DENSITY * tol[:, 8] + 8 * V64
    return tol


# ---------------------------------------------------------------- input recipes
def _upsample(coarse, shape):
    """trilinear, corners aligned: coarse (..., g, g, g) -> (..., D, H, W)"""
    out = coarse
    nd = out.ndim
    for axis, N in zip((nd - 3, nd - 2, nd - 1), shape):
        gsz = out.shape[axis]
        pos = np.linspace(0, gsz - 1, N)
        i0 = np.minimum(pos.astype(int), gsz - 2)
        w = (pos - i0).reshape([-1 if a == axis else 1 for a in range(nd)])
        out = np.take(out, i0, axis=axis) * (1 - w) + np.take(out, i0 + 1, axis=axis) * w
    return out


AMPLITUDE = 2.0   # voxels: the smooth field's largest component


def smooth_field(C, dims, seed, amplitude=AMPLITUDE):
    """(C,3,D,H,W) float32: a 4^3 lattice of uniform draws upsampled trilinearly, its largest magnitude `amplitude` (voxels)"""
    rng = np.random.default_rng(seed)
    f = _upsample(rng.uniform(-1, 1, size=(C, 3, 4, 4, 4)), dims)
    return np.ascontiguousarray(f * (amplitude / np.abs(f).max())).astype(np.float32)


def random_points(K, seed, reach=1.1):
    """(K,3) float32 uniform over [-reach, reach]^3"""
    return np.random.default_rng(seed).uniform(-reach, reach, size=(K, 3)).astype(np.float32)


SMOOTH_DIMS = ((5, 6, 7), (10, 14, 22))
SMOOTH_CHAINS = (1, 3)
SMOOTH_K = (1, 63, 64, 65, 257)
SMOOTH_SCALE = (1.75, 0.6, 2.5)   # a non-trivial per-channel scale of the mapped output


def smooth_case(dims, C, K):
    """-> (points (K,3), field (C,3,*dims), offset (K,3)) float32 of one smooth case of the GPU test"""
    seed = 7000 + 100 * SMOOTH_DIMS.index(tuple(dims)) + 10 * C + SMOOTH_K.index(K)
    pts = random_points(K, seed)
    offset = (np.random.default_rng(seed + 1).uniform(-30, 30, size=(K, 3))).astype(np.float32)
    return pts, smooth_field(C, dims, seed + 2), offset


def exact_case(dims, C=3, seed=0):
    """Inputs on which float32 arithmetic is exact (every n - 1 a power of two: tests/_exact_cases.EXACT_DIMS): field values
    multiples of 1/4 in [-8, 8]; for (2,3,5) every voxel centre, else 257 points on the quarter-cell lattice reaching half a
    cell past every face, the eight corners, points on faces and edges and the last voxel of each axis among them.
    -> (points (K,3) float32, field (C,3,*dims) float32, scale, offset (K,3) float32), scale and offset dyadic."""
    D, H, W = dims
    assert all(((n - 1) & (n - 2)) == 0 for n in dims), 'every dim must be 2^k + 1'
    rng = np.random.default_rng(9000 + seed)
    field = (rng.integers(-32, 33, size=(C, 3, D, H, W)) / 4.0).astype(np.float32)
    sizes = (W, H, D)
    if tuple(dims) == (2, 3, 5):
        z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
        idx = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float64)
    else:
        idx = np.stack([rng.integers(-2, 4 * (n - 1) + 3, size=257) / 4.0 for n in sizes], axis=1)
        special = []
        for cx in (0, W - 1):
            for cy in (0, H - 1):
                for cz in (0, D - 1):
                    special.append((cx, cy, cz))                                    # corners
        special += [(0, 1.25, 0.5), (W - 1, 0.75, 1.5), (1.5, 0, 0.25), (0.5, H - 1, 1.75), (1.25, 0.5, 0), (0.75, 1.5, D - 1)]  # faces
        special += [(0, 0, 0.5), (W - 1, H - 1, 1.25), (0.5, 0, D - 1), (W - 1, 1.5, 0)]                                        # edges
        special += [(W - 1, 1, 1), (1, H - 1, 1), (1, 1, D - 1), (W - 1.25, H - 1.5, D - 1.75)]                                 # last voxels
        idx[:len(special)] = np.asarray(special, dtype=np.float64)
    pts = np.stack([idx[:, c] * (2.0 / (n - 1)) - 1.0 for c, n in enumerate(sizes)], axis=1)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    scale = (0.5, 2.0, 4.0)
    offset = (rng.integers(-64, 65, size=pts.shape) / 2.0).astype(np.float32)
    return pts.astype(np.float32), field, scale, offset


# the recorder case of the GPU test: 5 records of 2 chains at 65 landmarks -> n = 10 Welford steps per landmark
RECORDER_DIMS, RECORDER_CHAINS, RECORDER_STEPS, RECORDER_K = (10, 14, 22), 2, 5, 65


def recorder_case():
    """-> (points (K,3), targets (K,3) float64 [-1,1] coordinates, displacements: list of (C,3,*dims) float32 in voxels: a
    smooth mean field of AMPLITUDE voxels plus, per record and chain, a smooth field of half a voxel).  Landmark 0 sits alone near the first corner, so that poisoning the voxels around it touches no other landmark."""
    rng = np.random.default_rng(4242)
    pts = rng.uniform(-0.6, 0.95, size=(RECORDER_K, 3))
    pts[0] = (-0.97, -0.96, -0.95)
    base = smooth_field(1, RECORDER_DIMS, 4243)[0]
    D, H, W = RECORDER_DIMS
    # the truth a fifth of a voxel or so off the landmark moved by the mean field: a Mahalanobis distance of order 1, not 100
    moved = sample(pts.astype(np.float32), base[None], np.float64)[0] / np.array([(W - 1) / 2, (H - 1) / 2, (D - 1) / 2])
    targets = pts + moved + rng.uniform(-0.02, 0.02, size=pts.shape)
    fields = [np.ascontiguousarray(base[None] + smooth_field(RECORDER_CHAINS, RECORDER_DIMS, 4244 + s, amplitude=0.5))
              for s in range(RECORDER_STEPS)]
    return pts, targets, fields
