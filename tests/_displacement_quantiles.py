"""The displacement credible intervals restated in numpy, and the inputs the tests share.

State for a volume (D,H,W) and B bins: `centre` (3,D,H,W) float32, the displacement of the first record, and `hist`
(3,B,D,H,W) counts.  Every record adds one count per voxel and channel a to the bin, in float32,

    t = floor((x_a - centre_a) * inv_width_a);  t = fmin(fmax(t, -B), B);  bin = min(max(int(t) + B / 2, 0), B - 1)

with width_a = float32(bin_width / scale_a) and inv_width_a = float32(1) / width_a.  numpy's float32 subtraction, product and
floor are the device's, and counts commute, so the device's histogram must equal `histogram_np` as integers.

The quantile of probability p after n records, with r = p n in double and b the first bin whose cumulative count >= r, is
scale_a (centre_a + ((b - B/2) + (r - cum_{b-1}) / count_b) width_a) in double, stored as float32; NaN where b is 0 or B - 1
(the open-ended bins).  The bin it lands in holds the order statistic x_(ceil(p n)), so it lies within one bin width of it:
`order_statistic` and `bound` are that independent check.  The tolerance is the one the feature was specified with:
bin_width (1 + 2^-20) plus 4 float32 ulps of |x_(k)| scale.
"""
import math

import numpy as np

MEAN_AMPLITUDE = 2.0  # voxels: the smooth mean field's largest component


def default_scale(shape):
    """normalised coordinates -> voxels for channels x, y, z of a (D, H, W) volume"""
    D, H, W = shape
    return ((W - 1) / 2, (H - 1) / 2, (D - 1) / 2)


def widths(bin_width, scale):
    """-> (width (3,) float32, inv_width (3,) float32), the inverse a float32 division"""
    w = np.array([np.float32(bin_width / s) for s in scale], dtype=np.float32)
    return w, (np.float32(1) / w).astype(np.float32)


def bins_np(x, centre, inv_width, B):
    """x, centre (3,...) float32, inv_width (3,) float32 -> the bins (3,...) int32, every step in float32"""
    x, centre = np.asarray(x, dtype=np.float32), np.asarray(centre, dtype=np.float32)
    iw = np.asarray(inv_width, dtype=np.float32).reshape((3,) + (1,) * (x.ndim - 1))
    with np.errstate(invalid='ignore', over='ignore'):
        d = x - centre
        assert d.dtype == np.float32
        t = np.floor(d * iw)
        assert t.dtype == np.float32
        t = np.fmin(np.fmax(t, np.float32(-B)), np.float32(B))  # fmax: a NaN gives -B
        return np.minimum(np.maximum(t.astype(np.int32) + B // 2, 0), B - 1)


def histogram_np(records, B, inv_width):
    """records (n,3,D,H,W) float32, the first one the centre -> (centre (3,D,H,W) float32, hist (3,B,D,H,W) int64)"""
    records = np.asarray(records, dtype=np.float32)
    centre = records[0].copy()
    hist = np.zeros((3, B) + records.shape[2:], dtype=np.int64)
    for x in records:
        b = bins_np(x, centre, inv_width, B)
        for a in range(3):
            np.put_along_axis(hist[a], b[a][None], np.take_along_axis(hist[a], b[a][None], axis=0) + 1, axis=0)
    return centre, hist


def finalize_np(centre, hist, n, width, scale, probs):
    """the finalize from a given state, in float64 -> quantiles (P,3,D,H,W), ci_width (D,H,W), rounded to float32 as the
    device stores them.  width: the (3,) float32 bin widths; scale: three floats, used as the float32 the ABI takes."""
    hist = np.asarray(hist).astype(np.int64)
    B = hist.shape[1]
    c = np.asarray(centre, dtype=np.float32).astype(np.float64)
    w = np.asarray(width, dtype=np.float32).astype(np.float64).reshape(3, 1, 1, 1)
    s = np.asarray(scale, dtype=np.float32).astype(np.float64).reshape(3, 1, 1, 1)
    cum = np.cumsum(hist, axis=1)
    out = []
    for p in probs:
        r = float(p) * n
        b = np.argmax(cum >= r, axis=1)  # the first bin whose cumulative count reaches r
        reached = np.take_along_axis(cum, b[:, None], axis=1)[:, 0] >= r
        count = np.take_along_axis(hist, b[:, None], axis=1)[:, 0]
        prev = np.take_along_axis(cum, b[:, None], axis=1)[:, 0] - count
        with np.errstate(invalid='ignore', divide='ignore'):
            q = s * (c + ((b - B // 2) + (r - prev) / count) * w)
        q[(b == 0) | (b == B - 1) | ~reached] = np.nan
        out.append(q.astype(np.float32))
    quantiles = np.stack(out)
    d = quantiles[-1].astype(np.float64) - quantiles[0].astype(np.float64)
    ci = np.sqrt((d ** 2).sum(axis=0))
    ci[np.isnan(quantiles).any(axis=(0, 1))] = np.nan
    return quantiles, ci.astype(np.float32)


def summary_np(n, hist, quantiles, ci_width, mask=None):
    """the summary over `mask` from the histogram and the given maps (float64 sums of whatever values they hold)"""
    hist = np.asarray(hist).astype(np.int64)
    q = np.asarray(quantiles, dtype=np.float64)
    ci = np.asarray(ci_width, dtype=np.float64)
    m = np.ones(ci.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    bad = np.isnan(q).any(axis=(0, 1))
    voxels, out = int(m.sum()), int((m & bad).sum())
    clipped = int((hist[:, 0] + hist[:, -1])[:, m].sum())
    ok = m & ~bad
    k = int(ok.sum())
    nan = float('nan')
    per = np.abs(q[-1] - q[0])
    mean = lambda v: float(v[ok].sum()) / k if k else nan
    return {'records': int(n), 'voxels': voxels, 'out_of_range_voxels': out, 'clipped_samples': clipped,
            'width_mean': mean(ci), 'width_max': float(ci[ok].max()) if k else nan,
            'width_x': mean(per[0]), 'width_y': mean(per[1]), 'width_z': mean(per[2]),
            'out_of_range_frac': out / voxels if voxels else nan,
            'clipped_frac': clipped / (3 * n * voxels) if voxels else nan}


def quantiles_np(records, probs, bins=64, bin_width=0.125, scale=None, mask=None):
    """records (n,3,D,H,W) float32 -> dict: centre, hist, width, inv_width, scale, quantiles, ci_width, summary"""
    records = np.asarray(records, dtype=np.float32)
    scale = default_scale(records.shape[2:]) if scale is None else tuple(float(s) for s in scale)
    w, iw = widths(bin_width, scale)
    centre, hist = histogram_np(records, bins, iw)
    q, ci = finalize_np(centre, hist, records.shape[0], w, scale, probs)
    return {'n': records.shape[0], 'centre': centre, 'hist': hist, 'width': w, 'inv_width': iw, 'scale': scale, 'quantiles': q,
            'ci_width': ci, 'summary': summary_np(records.shape[0], hist, q, ci, mask)}


def order_statistic(records, p, scale):
    """x_(ceil(p n)) of the scaled records per voxel and channel, float64 (3,D,H,W): numpy.sort, nothing of the histogram"""
    records = np.asarray(records, dtype=np.float32).astype(np.float64)
    n = records.shape[0]
    k = math.ceil(float(p) * n)
    s = np.asarray(scale, dtype=np.float64).reshape(1, 3, 1, 1, 1)
    return np.sort(records * s, axis=0)[k - 1]


def bound(x_k, bin_width):
    """the tolerance on |q - x_(k)|: one bin width, 2^-20 of it for the float32 bin edges, and 4 float32 ulps of |x_(k)|"""
    return bin_width * (1.0 + 2.0 ** -20) + 4.0 * np.spacing(np.abs(x_k).astype(np.float32)).astype(np.float64)


def check_bound(records, probs, quantiles, bin_width, scale, where=None):
    """|q - x_(ceil(p n))| <= bound at every voxel and channel of `where` (default: all); prints, then asserts.
    -> the worst error / tolerance"""
    worst = 0.0
    for j, p in enumerate(probs):
        x_k = order_statistic(records, p, scale)
        err = np.abs(np.asarray(quantiles[j], dtype=np.float64) - x_k)
        tol = bound(x_k, bin_width)
        sel = np.ones(err.shape, dtype=bool) if where is None else np.broadcast_to(where, err.shape)
        assert np.isfinite(err[sel]).all(), f'p = {p}: a quantile that should be in range is not finite'
        if sel.any():
            worst = max(worst, float((err[sel] / tol[sel]).max()))
        assert (err[sel] <= tol[sel]).all(), (p, float(err[sel].max()), float((err[sel] / tol[sel]).max()))
    print({'quantile against the order statistic, worst error / tolerance': worst})
    return worst


def check_monotone(quantiles):
    """non-decreasing in p wherever both neighbours are finite"""
    q = np.asarray(quantiles, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        assert not (q[1:] < q[:-1]).any()


# ---------------------------------------------------------------- inputs
def _upsample(coarse, shape):
    """trilinear, corners aligned: coarse (c, g, g, g) -> (c, D, H, W)"""
    out = coarse
    for axis, N in zip((1, 2, 3), shape):
        g = out.shape[axis]
        pos = np.linspace(0.0, g - 1.0, N)
        lo = np.minimum(pos.astype(int), g - 2)
        f = (pos - lo).reshape([-1 if i == axis else 1 for i in range(4)])
        out = np.take(out, lo, axis=axis) * (1 - f) + np.take(out, lo + 1, axis=axis) * f
    return out


def draw_records(n, shape, seed, noise=0.5):
    """n records (n, 3, D, H, W) float32, normalised coordinates: a smooth mean field of MEAN_AMPLITUDE voxels plus, per
    record, white noise N(0, 1) * `noise` voxels * a smooth amplitude field in [0.01, 1] (a posterior is tight in some places
    and wide in others)"""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    mean = _upsample(rng.uniform(-MEAN_AMPLITUDE, MEAN_AMPLITUDE, size=(3, 3, 3, 3)), shape)
    amp = _upsample(rng.uniform(0.1, 1.0, size=(1, 3, 3, 3)) ** 2, shape)
    vox = mean[None] + noise * amp[None] * rng.standard_normal((n, 3) + tuple(shape))
    to_norm = np.array([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)]).reshape(1, 3, 1, 1, 1)
    return (vox * to_norm).astype(np.float32)


def hand_checked_records(shape=(3, 4, 5), width=0.5):
    """centre + {0, 1, 2, 3} * width / 2 at every voxel, the centre a different multiple of 1/4 per voxel and channel:
    two records in the centre's bin and two in the next one, everything exact in float32"""
    D, H, W = shape
    idx = np.arange(3 * D * H * W).reshape((3,) + tuple(shape))
    centre = ((idx % 23) - 11) * 0.25
    return np.stack([centre + k * width / 2 for k in range(4)]).astype(np.float32), centre


# hand-checked: scale (2, 2, 2), bin_width 1 -> width 0.5; n = 4; r = 1, 2, 3 for p = 1/4, 1/2, 3/4; the centre's bin holds
# records 1-2 and the next one records 3-4: q = 2 (c + 0.25), 2 (c + 0.5), 2 (c + 0.75); the band is 1 wide per channel
HAND_SCALE, HAND_BIN_WIDTH, HAND_PROBS, HAND_OFFSETS, HAND_CI = (2.0, 2.0, 2.0), 1.0, (0.25, 0.5, 0.75), (0.25, 0.5, 0.75), math.sqrt(3.0)

# C, steps, shape, bins: the minimum; every path of the update (first record, one and several chains, chains sharing a bin);
# an odd W longer than a wavefront with more than one block; the smallest and the largest bin count
CASES = [
    (1, 1, (2, 2, 3), 4),
    (2, 3, (3, 4, 5), 16),
    (3, 2, (5, 7, 9), 64),
    (2, 20, (3, 5, 131), 64),
    (1, 3, (4, 5, 6), 256),
]
# C, steps, shape, bins with noise 0.5 voxels and bin_width 0.125: every quantile of PROBS is inside the bins (checked on
# the CPU by test_displacement_quantiles_host.py)
IN_RANGE_CASES = [
    (2, 20, (5, 7, 9), 64),
    (8, 25, (4, 5, 6), 64),
    (2, 20, (3, 5, 131), 64),
    (1, 3, (4, 5, 6), 256),
]
# 60 records with noise 2.0 voxels in 16 bins of 0.125 (one voxel either side of the centre): where the noise is at its widest
# every voxel has a quantile in an open-ended bin, where it is tight none has
CLIP_CASE = (3, 20, (8, 12, 15), 16)
CLIP_NOISE = 2.0
PROBS = (0.05, 0.5, 0.95)
BIN_WIDTH = 0.125


def case_seed(C, steps, shape, bins):
    return C * 1000 + steps * 100 + shape[2] + bins


def case_mask(shape):
    return np.random.default_rng(shape[2]).random(shape) < 0.6
