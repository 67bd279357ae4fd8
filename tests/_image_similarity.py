"""CPU restatement of the intensity-similarity operator ("Intensity similarity") in numpy, and the input
builders of its tests.  It shares no code with the HIP path.

Binning in float32, in exactly the operations of the definition -- inv_w = float32(B) / (hi - lo), t = (x - lo) * inv_w,
b = min(B - 1, max(0, floor(t))) -- so every count is reproduced; np.bincount for the histogram; float64 sums and entropies."""
import numpy as np

COLUMNS = ('n', 'n_nonfinite', 'n_clipped', 'mse', 'ncc', 'h_fixed', 'h_moving', 'h_joint', 'mi', 'nmi')
F32 = np.float32


def bin_index(x, lo, hi, bins):
    """-> (bin of every value of the float32 array x, whether it lies outside [lo, hi]); x must be finite"""
    x = np.asarray(x, dtype=F32)
    lo, hi = F32(lo), F32(hi)
    inv_w = F32(bins) / (hi - lo)
    with np.errstate(over='ignore'):  # a finite value far outside the range: t = inf, the last bin
        t = (x - lo) * inv_w
    assert t.dtype == F32
    b = np.minimum(F32(bins - 1), np.maximum(F32(0), np.floor(t))).astype(np.int64)
    return b, (x < lo) | (x > hi)


def entropy(counts, n):
    """-sum p ln p over the non-zero counts, p = count / n, in float64"""
    c = np.asarray(counts, dtype=np.float64).ravel()
    p = c[c > 0] / float(n)
    return float(-(p * np.log(p)).sum())


def reference_one(f, m, mask, bins, f_range, m_range):
    """one chain: f, m float32 arrays of one shape, mask bool / uint8 of that shape or None -> (hist (bins,bins) int64, stats
    dict keyed by COLUMNS)"""
    f, m = np.asarray(f, dtype=F32).ravel(), np.asarray(m, dtype=F32).ravel()
    inside = np.ones(f.shape, bool) if mask is None else np.asarray(mask).ravel() != 0
    finite = np.isfinite(f) & np.isfinite(m)
    take = inside & finite
    ft, mt = f[take], m[take]
    n = int(take.sum())
    bf, cf = bin_index(ft, *f_range, bins)
    bm, cm = bin_index(mt, *m_range, bins)
    hist = np.bincount(bf * bins + bm, minlength=bins * bins).reshape(bins, bins)
    st = dict(n=n, n_nonfinite=int((inside & ~finite).sum()), n_clipped=int((cf | cm).sum()))
    nan = float('nan')
    if n == 0:
        st.update({k: nan for k in COLUMNS[3:]})
        return hist, st
    fd, md = ft.astype(np.float64), mt.astype(np.float64)
    st['mse'] = float(((fd - md) ** 2).sum() / n)
    mean_f, mean_m = fd.sum() / n, md.sum() / n
    var_f, var_m = (fd * fd).sum() / n - mean_f * mean_f, (md * md).sum() / n - mean_m * mean_m
    st['ncc'] = float(((fd * md).sum() / n - mean_f * mean_m) / np.sqrt(var_f * var_m)) if var_f > 0 and var_m > 0 else nan
    hf, hm, hj = entropy(hist.sum(axis=1), n), entropy(hist.sum(axis=0), n), entropy(hist, n)
    st.update(h_fixed=hf, h_moving=hm, h_joint=hj, mi=hf + hm - hj, nmi=(hf + hm) / hj if hj != 0 else nan)
    return hist, st


def reference(fixed, moving, mask, bins, f_range, m_range):
    """fixed (Cf,1,D,H,W), moving (C,1,D,H,W), mask (1,1,D,H,W) or None -> (hist (C,bins,bins) int64, stats (C,10) float64)"""
    C = moving.shape[0]
    hists, rows = [], []
    for c in range(C):
        h, st = reference_one(fixed[c if fixed.shape[0] > 1 else 0, 0], moving[c, 0], None if mask is None else mask[0, 0], bins,
                              f_range, m_range)
        hists.append(h)
        rows.append([st[k] for k in COLUMNS])
    return np.stack(hists), np.array(rows, dtype=np.float64)


# ---------------------------------------------------------------- input builders
def random_pair(shape, C, Cf, seed):
    """uniform random fixed image(s) in [0, 1) and moving = 0.7 f + 0.3 noise, float32"""
    rng = np.random.default_rng(seed)
    fixed = rng.random((Cf, 1, *shape), dtype=F32)
    noise = rng.random((C, 1, *shape), dtype=F32)
    moving = (F32(0.7) * np.broadcast_to(fixed, noise.shape) + F32(0.3) * noise).astype(F32)
    return fixed, moving


def random_mask(shape, seed, dtype=bool):
    rng = np.random.default_rng(seed)
    return (rng.random((1, 1, *shape)) < 0.5).astype(dtype)


def spoil(fixed, moving, seed):
    """a few NaN / Inf voxels and values beyond [0, 1] in every volume of copies of the pair"""
    rng = np.random.default_rng(seed)
    fixed, moving = fixed.copy(), moving.copy()
    for vol in fixed:
        flat = vol.reshape(-1)
        i = rng.choice(flat.size, 8, replace=False)
        flat[i[0:2]], flat[i[2]], flat[i[3]] = np.nan, np.inf, -np.inf
        flat[i[4:8]] = F32([1.25, -0.5, 3e38, -1e-6])
    for vol in moving:
        flat = vol.reshape(-1)
        j = rng.choice(flat.size, 8, replace=False)
        flat[j[0]], flat[j[1:3]], flat[j[3]] = np.nan, np.inf, -np.inf
        flat[j[4:8]] = F32([1.0000001, -2.0, -3e38, 7.0])
    return fixed, moving


def lattice(bins=8, repeats=5):
    """independent images: f = ((i mod B) + 1/2) / B, m = ((floor(i / B) mod B) + 1/2) / B over V = repeats B^2 voxels; every joint
    cell of the [0, 1] histogram holds exactly `repeats`"""
    i = np.arange(repeats * bins * bins)
    f = ((i % bins) + 0.5) / bins
    m = (((i // bins) % bins) + 0.5) / bins
    return f.astype(F32), m.astype(F32)


EDGE_VALUES = F32([0.0, 0.125, 0.25 - 2.0 ** -26, 0.25, 1.0, 1.5, -0.3, 0.999999])
EDGE_BINS = [0, 1, 1, 2, 7, 7, 0, 7]  # range [0, 1], 8 bins; 1.5 and -0.3 are clipped
