"""numpy restatement of the Jacobian posterior ("Jacobian posterior"), the input recipes and the
tolerances, shared by the host and GPU tests.

Rounding bound `e` of a float32 evaluation of det.  u = 2^-24 is the unit roundoff.  The inputs are float32 and exact.
  spacing 2 / (N - 1)                 1 rounding   (N - 1 is an exact float)
  forward difference a - b            1 rounding
  quotient difference / spacing       1 rounding   -> every entry of nabla carries (1 + u)^3
  a product of three entries          2 roundings  -> every one of the six products carries (1 + u)^(3 * 3 + 2) = (1 + u)^11
  the sum of the six products         5 additions  -> every product passes through at most 5 of them
so |det32 - det| <= gamma_16 * S with S the sum of the absolute six products and gamma_16 = 16 u / (1 - 16 u).  A fused
multiply-add drops roundings and never adds one, so the bound holds whatever the compiler contracts.
"""
import numpy as np

U = 2.0 ** -24
GAMMA16 = 16 * U / (1 - 16 * U)
DELTA = 1e-3   # |det| below this: the sign of a float32 det is not pinned, the voxel-record is "in the band"
FACTOR = 2.0   # over the first-order tolerances below: -ln(1 - r) <= 2 r for the r = e / |det| <= 1/2 outside the band


def nabla_np(t, dtype=np.float64):
    """t (..., 3, D, H, W) float32 -> n[a][comp] (..., D, H, W) of dtype: forward differences with the last one replicated,
    divided by the normalised spacing 2 / (N - 1); a = 0, 1, 2 is the W, H, D axis, comp the x, y, z channel"""
    t = np.asarray(t, dtype=np.float32).astype(dtype)
    n = [[None] * 3 for _ in range(3)]
    for a, axis in enumerate((-1, -2, -3)):
        N = t.shape[axis]
        sp = dtype(2.0) / dtype(N - 1)
        d = np.diff(t, axis=axis)
        last = np.take(d, [-1], axis=axis)
        d = np.concatenate([d, last], axis=axis) / sp
        for comp in range(3):
            n[a][comp] = d[..., comp, :, :, :]
    return n


def det_np(t, dtype=np.float64):
    """-> (det, S): the six-product formula in the kernel's order, and the sum of the absolute products"""
    n = nabla_np(t, dtype)
    p = [n[0][0] * n[1][1] * n[2][2], n[0][1] * n[1][2] * n[2][0], n[0][2] * n[1][0] * n[2][1],
         n[2][0] * n[1][1] * n[0][2], n[2][1] * n[1][2] * n[0][0], n[2][2] * n[1][0] * n[0][1]]
    det = p[0] + p[1] + p[2] - p[3] - p[4] - p[5]
    S = sum(np.abs(x) for x in p)
    return det, S


def maps_np(folds, mean, m2, n):
    """the final maps from the state, float64: fold_prob, logJ_mean, logJ_std (NaN where no record is valid)"""
    folds = np.asarray(folds).astype(np.int64)
    k = n - folds
    with np.errstate(invalid='ignore', divide='ignore'):
        std = np.sqrt(np.asarray(m2, dtype=np.float64) / np.maximum(k - 1, 1))
    return folds / n, np.where(k >= 1, np.asarray(mean, dtype=np.float64), np.nan), np.where(k >= 1, std, np.nan)


def summary_np(folds, n, fold_prob, logJ_mean, logJ_std, mask=None):
    """the summary over `mask` of the given maps (float64 sums of whatever values they hold)"""
    folds = np.asarray(folds).astype(np.int64)
    m = np.ones(folds.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    voxels = int(m.sum())
    f = folds[m]
    valid = f < n
    nan = float('nan')
    lm = np.asarray(logJ_mean, dtype=np.float64)[m][valid]
    ls = np.asarray(logJ_std, dtype=np.float64)[m][valid]
    fp = np.asarray(fold_prob, dtype=np.float64)[m]
    some = bool(valid.any())
    return {'records': int(n), 'voxels': voxels, 'folded_voxels': int((f > 0).sum()), 'always_folded': int((f >= n).sum()),
            'fold_records': int(f.sum()),
            'fold_prob_max': float(fp.max()) if voxels else nan,
            'fold_prob_mean': float(f.sum()) / (n * voxels) if voxels else nan,
            'logJ_mean_min': float(lm.min()) if some else nan, 'logJ_mean_max': float(lm.max()) if some else nan,
            'logJ_std_mean': float(ls.sum() / valid.sum()) if some else nan, 'logJ_std_max': float(ls.max()) if some else nan}


def jacobian_posterior_np(records, mask=None):
    """records (n, 3, D, H, W) float32 in record order (steps, chains within a step) -> dict: det, e (n,D,H,W) float64 (e the
    forward bound of the module docstring), folds, k (D,H,W) int64, mean, m2 (two-pass moments of log det over the records
    with det > 0; 0 where there is none), fold_prob, logJ_mean, logJ_std (D,H,W) float64, summary (of the float64 maps)."""
    records = np.asarray(records, dtype=np.float32)
    n = records.shape[0]
    det, S = det_np(records)
    e = GAMMA16 * S
    folded = ~(det > 0)
    folds = folded.sum(axis=0).astype(np.int64)
    k = n - folds
    with np.errstate(invalid='ignore', divide='ignore'):
        x = np.where(folded, 0.0, np.log(np.where(folded, 1.0, det)))
        mean = np.where(k > 0, x.sum(axis=0) / np.maximum(k, 1), 0.0)
    m2 = np.where(folded, 0.0, (x - mean) ** 2).sum(axis=0)
    fold_prob, logJ_mean, logJ_std = maps_np(folds, mean, m2, n)
    return {'n': n, 'det': det, 'e': e, 'x': x, 'folded': folded, 'folds': folds, 'k': k, 'mean': mean, 'm2': m2,
            'fold_prob': fold_prob, 'logJ_mean': logJ_mean, 'logJ_std': logJ_std,
            'summary': summary_np(folds, n, fold_prob, logJ_mean, logJ_std, mask)}


def fold_bounds(det, delta=DELTA):
    """per voxel, the fold counts a float32 evaluation may give: #(det <= -delta) <= folds <= #(det < delta); NaN counts in both"""
    nan = np.isnan(det)
    return ((det <= -delta) | nan).sum(axis=0), ((det < delta) | nan).sum(axis=0)


def tolerances(ref, delta=DELTA):
    """-> (clear, tol_mean, tol_root_m2, tol_std), all (D,H,W).  `clear`: voxels none of whose records has |det| < delta;
    the tolerances mean something there only.  Per valid record the float32 log det is off by at most
        a_r = e_r / det_r + 2 u |x_r|        (e propagated through the log to first order; logf within 1 ulp <= 2 u |x|).
    With X = max |x_r|, R = max x_r - min x_r and k valid records, the float32 Welford recurrences add
      mean: err_k <= (1 - 1/k) err_{k-1} + u (2 R / k + X)  [d and d / k round an |.| <= R, the sum an |.| <= X]
            => E_m = u (2 R + X (k + 1) / 2)
      M2:   each term d (x - mean_k) carries 2 R E_m + 3 u R^2, each addition u M2  => dM2 = k (2 R E_m + 3 u R^2 + u M2)
    and sqrt(M2) = |x - mean| is a norm of the records, so the a_r move it by at most |a|_2, and |sqrt(p) - sqrt(q)| <=
    min(|p - q| / sqrt(q), sqrt(|p - q|)).  logJ_std divides by sqrt(max(k - 1, 1)) and takes two more roundings.
    Everything is multiplied by FACTOR."""
    det, e, x, folded, k, m2 = ref['det'], ref['e'], ref['x'], ref['folded'], ref['k'], ref['m2']
    clear = ~(np.abs(det) < delta).any(axis=0) & ~np.isnan(det).any(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        a = np.where(folded, 0.0, e / np.where(folded, 1.0, det) + 2 * U * np.abs(x))
        kk = np.maximum(k, 1)
        X = np.abs(x).max(axis=0)
        R = np.where(folded, -np.inf, x).max(axis=0) - np.where(folded, np.inf, x).min(axis=0)
        R = np.where(k > 0, R, 0.0)
        E_m = U * (2 * R + X * (kk + 1) / 2)
        tol_mean = FACTOR * (a.sum(axis=0) / kk + E_m)
        dM2 = kk * (2 * R * E_m + 3 * U * R * R + U * m2)
        root = np.sqrt(m2)
        rounding = np.minimum(np.where(root > 0, dM2 / np.where(root > 0, root, 1.0), np.inf), np.sqrt(dM2))
        tol_root = FACTOR * (np.sqrt((a * a).sum(axis=0)) + rounding)
        tol_std = tol_root / np.sqrt(np.maximum(k - 1, 1)) + FACTOR * 2 * U * np.sqrt(m2 / np.maximum(k - 1, 1))
    return clear, tol_mean, tol_root, tol_std


def welford_f32(det32):
    """the update kernel's recurrences in float32 numpy (no fused multiply-add), records in order:
    det32 (n,D,H,W) float32 -> folds int32, mean, m2 float32"""
    det32 = np.asarray(det32, dtype=np.float32)
    shape = det32.shape[1:]
    folds = np.zeros(shape, dtype=np.int32)
    k = np.zeros(shape, dtype=np.int32)
    mean = np.zeros(shape, dtype=np.float32)
    m2 = np.zeros(shape, dtype=np.float32)
    for det in det32:
        bad = ~(det > 0)
        with np.errstate(invalid='ignore', divide='ignore'):
            v = np.log(np.where(bad, 1.0, det.astype(np.float64))).astype(np.float32)  # a correctly rounded logf
        folds += bad
        k += ~bad
        first = ~bad & (k == 1)
        d = (v - mean).astype(np.float32)
        new_mean = (mean + (d / np.maximum(k, 1).astype(np.float32)).astype(np.float32)).astype(np.float32)
        new_m2 = (m2 + (d * (v - new_mean).astype(np.float32)).astype(np.float32)).astype(np.float32)
        mean = np.where(bad, mean, np.where(first, v, new_mean)).astype(np.float32)
        m2 = np.where(bad, m2, np.where(first, np.float32(0), new_m2)).astype(np.float32)
    return folds, mean, m2


# ---------------------------------------------------------------- input recipes
def identity_np(shape):
    """(3, D, H, W) float32: the identity transformation in normalised coordinates, channels x (W), y (H), z (D)"""
    D, H, W = shape
    z, y, x = np.meshgrid(np.linspace(-1, 1, D), np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing='ij')
    return np.stack([x, y, z]).astype(np.float32)


def _upsample(coarse, shape):
    """trilinear, corners aligned: coarse (3, g, g, g) -> (3, D, H, W)"""
    out = coarse
    for axis, N in zip((1, 2, 3), shape):
        g = out.shape[axis]
        pos = np.linspace(0, g - 1, N)
        i0 = np.minimum(pos.astype(int), g - 2)
        w = (pos - i0).reshape([-1 if a == axis else 1 for a in range(4)])
        out = np.take(out, i0, axis=axis) * (1 - w) + np.take(out, i0 + 1, axis=axis) * w
    return out


def _voxels_to_normalised(d, shape):
    D, H, W = shape
    scale = np.array([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)]).reshape(3, 1, 1, 1)
    return d * scale


def smooth_displacement(rng, shape, amplitude):
    """a 4 x 4 x 4 grid of uniform draws, trilinearly upsampled, its largest component `amplitude` voxels"""
    d = _upsample(rng.uniform(-1, 1, size=(3, 4, 4, 4)), shape)
    return _voxels_to_normalised(d * (amplitude / np.abs(d).max()), shape)


def white_displacement(rng, shape, amplitude):
    """independent uniform draws in [-amplitude, amplitude] voxels"""
    return _voxels_to_normalised(rng.uniform(-amplitude, amplitude, size=(3, *shape)), shape)


def draw_records(recipe, n, shape, seed):
    """n records (n, 3, D, H, W) float32.  'smooth': identity + a smooth displacement of 1.5 voxels (no folds on the larger
    volumes).  'folding': per record one of identity + 4 voxels smooth, + 0.6 voxels white noise, + 1.5 voxels white noise,
    in turn from a drawn start."""
    rng = np.random.default_rng(seed)
    ident = identity_np(shape).astype(np.float64)
    out = []
    start = int(rng.integers(3))
    for r in range(n):
        if recipe == 'smooth':
            d = smooth_displacement(rng, shape, 1.5)
        elif recipe == 'folding':
            kind = (start + r) % 3
            d = smooth_displacement(rng, shape, 4.0) if kind == 0 else white_displacement(rng, shape, (0.6, 1.5)[kind - 1])
        else:
            raise ValueError(recipe)
        out.append((ident + d).astype(np.float32))
    return np.stack(out)


# C, steps, shape: every chain count, 1 to 5 steps, 2 x 2 x 3 to 64^3, odd widths and widths that are no multiple of 64
CASES = [
    (1, 1, (2, 2, 3)),
    (2, 3, (3, 4, 5)),
    (3, 2, (5, 7, 9)),
    (8, 1, (5, 7, 9)),
    (2, 5, (17, 16, 33)),
    (1, 4, (9, 6, 70)),
    (3, 3, (32, 32, 32)),
    (8, 2, (24, 40, 65)),
    (2, 2, (64, 64, 64)),
]
RECIPES = ('smooth', 'folding')


def case_seed(C, steps, shape, recipe):
    return C * 1000 + steps * 100 + shape[2] + (7 if recipe == 'folding' else 0)
