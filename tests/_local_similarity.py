"""CPU restatement of the local-similarity operator ("Local similarity maps") in float64 numpy, the
error bounds its device tests hold the kernel to, and their input builders.  It shares no code with the HIP path or with
ops.py, except ops.local_similarity_constants, which turns the two intensity ranges into the four constants.

Windows by np.pad(mode='edge') and shifted adds, one axis after the other.  A non-finite value is replaced by 0 before the
sums and counted in a window sum of its own, so it spoils exactly the voxels whose clamped window holds it."""
import numpy as np

COLUMNS = ('n', 'n_flat', 'n_nonfinite', 'lncc_mean', 'lncc_min', 'ssim_mean', 'ssim_min')
UNIT = (0.0, 1.0)


def box_sum(a, r):
    """sum over the (2r+1)^3 window with clamped indices, of a 3-D float64 array"""
    a = np.pad(np.asarray(a, dtype=np.float64), r, mode='edge')
    for axis in range(3):
        n = a.shape[axis] - 2 * r
        acc = np.zeros_like(np.take(a, range(n), axis=axis))
        for s in range(2 * r + 1):
            acc = acc + np.take(a, range(s, s + n), axis=axis)
        a = acc
    return a


def reference_maps(f, m, r, consts):
    """one chain: f, m float32 arrays (D,H,W); consts = (floor_f, floor_m, c1, c2) -> dict of float64 (D,H,W) arrays: 'lncc',
    'ssim' (NaN where undefined), 'finite', 'flat' (bool) and the moments the error bounds are made of"""
    floor_f, floor_m, c1, c2 = consts
    f, m = np.asarray(f, dtype=np.float32), np.asarray(m, dtype=np.float32)
    bad = ~(np.isfinite(f) & np.isfinite(m))
    f64, m64 = np.where(bad, 0.0, f.astype(np.float64)), np.where(bad, 0.0, m.astype(np.float64))
    n = float((2 * r + 1) ** 3)
    finite = box_sum(bad, r) == 0
    mu_f, mu_m = box_sum(f64, r) / n, box_sum(m64, r) / n
    e_ff, e_mm, e_fm = box_sum(f64 * f64, r) / n, box_sum(m64 * m64, r) / n, box_sum(f64 * m64, r) / n
    var_f, var_m = np.maximum(e_ff - mu_f * mu_f, 0.0), np.maximum(e_mm - mu_m * mu_m, 0.0)
    cov = e_fm - mu_f * mu_m
    flat = ~((var_f > floor_f) & (var_m > floor_m))
    with np.errstate(divide='ignore', invalid='ignore'):
        lncc = np.clip(cov / np.sqrt(var_f * var_m), -1.0, 1.0)
    ssim = ((2.0 * mu_f * mu_m + c1) * (2.0 * cov + c2)) / ((mu_f * mu_f + mu_m * mu_m + c1) * (var_f + var_m + c2))
    nan = np.nan
    return {'lncc': np.where(finite & ~flat, lncc, nan), 'ssim': np.where(finite, ssim, nan), 'finite': finite, 'flat': flat & finite,
            'n': n, 'e_ff': e_ff, 'e_mm': e_mm, 'var_f': var_f, 'var_m': var_m, 'b1': mu_f * mu_f + mu_m * mu_m + c1,
            'b2': var_f + var_m + c2}


def reference_stats(maps, mask=None):
    """the seven statistics of one chain's reference_maps over the mask (bool / uint8 (D,H,W), or None) -> dict by COLUMNS"""
    inside = np.ones(maps['finite'].shape, bool) if mask is None else np.asarray(mask).reshape(maps['finite'].shape) != 0
    fin = inside & maps['finite']
    defined = fin & ~maps['flat']
    lv, sv = maps['lncc'][defined], maps['ssim'][fin]
    return {'n': int(fin.sum()), 'n_flat': int((fin & maps['flat']).sum()), 'n_nonfinite': int((inside & ~maps['finite']).sum()),
            'lncc_mean': float(lv.mean()) if lv.size else float('nan'), 'lncc_min': float(lv.min()) if lv.size else float('inf'),
            'ssim_mean': float(sv.mean()) if sv.size else float('nan'), 'ssim_min': float(sv.min()) if sv.size else float('inf')}


def lncc_bound(maps):
    """per voxel: 2^-23 |ref| + 4 n 2^-52 (E_ff / var_f + E_mm / var_m) -- test_gpu_local_similarity.py derives it"""
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = maps['e_ff'] / maps['var_f'] + maps['e_mm'] / maps['var_m']
    return 2.0 ** -23 * np.abs(maps['lncc']) + 4.0 * maps['n'] * 2.0 ** -52 * ratio


def ssim_bound(maps):
    """per voxel: 2^-23 |ref| + 4 n 2^-52 (E_ff + E_mm) (1 / B1 + 1.5 / B2), B1 = mu_f^2 + mu_m^2 + c1, B2 = var_f + var_m + c2"""
    total = maps['e_ff'] + maps['e_mm']
    return 2.0 ** -23 * np.abs(maps['ssim']) + 4.0 * maps['n'] * 2.0 ** -52 * total * (1.0 / maps['b1'] + 1.5 / maps['b2'])


def noise_pair(shape, chains, seed):
    """-> fixed, moving (chains,1,D,H,W) float32: uniform noise in [0,1) and moving = 0.6 fixed + 0.4 noise, chain by chain"""
    rng = np.random.default_rng(seed)
    f = rng.random((chains, 1) + tuple(shape)).astype(np.float32)
    m = (0.6 * f + 0.4 * rng.random(f.shape)).astype(np.float32)
    return f, m


def random_mask(shape, seed, dtype=bool):
    """about two voxels of three set"""
    return (np.random.default_rng(seed).random(tuple(shape)) < 0.67).astype(dtype)
