"""numpy restatement of the posterior label maps, shared by the host and GPU tests."""
import math

import numpy as np

BINS = 10


def label_posterior_np(records, seg_fixed, labels, mask=None):
    """records (n, D, H, W) int, in record order (steps, chains within a step); seg_fixed (D, H, W); labels: K distinct
    values; mask (D, H, W) bool or None.  -> dict of counts (K,D,H,W) int64, entropy (D,H,W) float64, map (D,H,W) int64,
    summary (K, 6 + 3 BINS) int64, vol (n, K) int64, vol_mean / vol_m2 (K,) float64, entropy_voxels / sum / max (over the
    float32-rounded entropy) and inconsistent (always 0 here)."""
    records = np.asarray(records)
    n = records.shape[0]
    K = len(labels)
    lab = np.asarray(labels).reshape(K, 1, 1, 1)
    hit = records[:, None] == lab[None]                      # (n, K, D, H, W)
    counts = hit.sum(axis=0).astype(np.int64)                # (K, D, H, W)
    other = n - counts.sum(axis=0)
    classes = np.concatenate([other[None], counts])          # (K + 1, D, H, W): other first
    c = classes.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        clnc = np.where(classes > 0, c * np.log(np.where(classes > 0, c, 1.0)), 0.0)
    entropy = math.log(n) - clnc.sum(axis=0) / n
    entropy = np.maximum(entropy, 0.0)
    best = classes.argmax(axis=0)                            # first maximum: other, then structure order
    map_label = np.where(best == 0, 0, np.asarray(labels)[np.maximum(best - 1, 0)])
    y = seg_fixed[None] == lab                               # (K, D, H, W)
    summary = np.zeros((K, 6 + 3 * BINS), dtype=np.int64)
    for j in range(K):
        cj, yj = counts[j].reshape(-1), y[j].reshape(-1)
        mj = (best - 1 == j).reshape(-1)
        summary[j, :6] = [yj.sum(), cj.sum(), (cj * yj).sum(), mj.sum(), (mj & yj).sum(), ((cj > 0) & (cj < n)).sum()]
        pair = (cj > 0) | yj
        b = np.minimum(cj[pair] * BINS // n, BINS - 1)
        for bb in range(BINS):
            sel = b == bb
            summary[j, 6 + 3 * bb: 9 + 3 * bb] = [sel.sum(), cj[pair][sel].sum(), yj[pair][sel].sum()]
    vol = hit.reshape(n, K, -1).sum(axis=2).astype(np.int64)
    mean, m2 = np.zeros(K), np.zeros(K)
    for k in range(1, n + 1):  # Welford in record order, as the device folds it
        x = vol[k - 1].astype(np.float64)
        d = x - mean
        mean = mean + d / k
        m2 = m2 + d * (x - mean)
    sel = np.ones(entropy.shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    e32 = entropy.astype(np.float32).astype(np.float64)[sel]
    return {'counts': counts, 'entropy': entropy, 'map': map_label, 'summary': summary, 'vol': vol, 'vol_mean': mean,
            'vol_m2': m2, 'entropy_voxels': int(sel.sum()), 'entropy_sum': float(e32.sum()),
            'entropy_max': float(e32.max()) if e32.size else 0.0, 'n': n}


def derived_np(ref, spacing=(1.0, 1.0, 1.0)):
    """the Python-side quantities of DESIGN.md section 6 from label_posterior_np's output -> (per-structure list of dicts,
    pooled ECE, entropy mean, entropy max)"""
    n, s = ref['n'], ref['summary'].astype(np.float64)
    v = float(np.prod(spacing))
    out = []
    nan = float('nan')
    for j in range(s.shape[0]):
        S0, S1, S2, S3, S4, S5 = s[j, :6]
        bins = s[j, 6:].reshape(BINS, 3)
        pairs = bins[:, 0].sum()
        out.append({'soft_DSC': 2 * S2 / (S1 + n * S0) if S1 + n * S0 else nan,
                    'DSC_MAP': 2 * S4 / (S3 + S0) if S3 + S0 else nan,
                    'vol_mean': ref['vol'][:, j].mean() * v,
                    'vol_std': math.sqrt(((ref['vol'][:, j] - ref['vol'][:, j].mean()) ** 2).sum() / max(n - 1, 1)) * v,
                    'uncertain_vol': S5 * v,
                    'ECE': np.abs(bins[:, 1] / n - bins[:, 2]).sum() / pairs if pairs else nan})
    pooled = s[:, 6:].reshape(-1, BINS, 3).sum(axis=0)
    pairs = pooled[:, 0].sum()
    ece = np.abs(pooled[:, 1] / n - pooled[:, 2]).sum() / pairs if pairs else nan
    vox = ref['entropy_voxels']
    return out, ece, (ref['entropy_sum'] / vox if vox else nan), (ref['entropy_max'] if vox else nan)
