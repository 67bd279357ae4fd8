"""numpy float64 restatement of the structure report ("Structure report"): the two labelled reductions,
the host summary, the label-volume recipes and the tolerances, shared by the host and GPU tests.

det J and its forward rounding bound `e` come from tests/_jacobian_posterior.py (the device forms det in float32: |det32 - det|
<= e).  The reference sums are formed in extended precision (np.longdouble, 64 bits of mantissa on x86: their own error is 2^-11
of the bounds below), so a bound on the device's error is a bound on the difference:
  counts                       exact
  a double sum of m terms      m 2^-53 sum |term|, whatever the order (every partial sum is at most sum |term|)
  sum det                      that, plus FACTOR sum e over the structure
  min / max det                the largest e of the structure
  max |w|                      2 ulp of double
  folded                       between #(det <= -DELTA) and #(det < DELTA) over the structure, NaN counted in both
The terms w_c, |w|^2 and |w| themselves are the device's bits: w_c is an exact product, and |w|^2 = (w_x^2 + w_y^2) + w_z^2 and
its correctly rounded square root are rounded operation by operation on both sides.
"""
import math

import numpy as np

from tests._jacobian_posterior import DELTA, FACTOR, draw_records, fold_bounds, identity_np, jacobian_posterior_np  # noqa: F401

EPS = 2.0 ** -53
MOTION_INTS, MOTION_FLOATS, MAP_INTS, MAP_FLOATS = 2, 9, 2, 4
SUM_COLUMNS = (0, 1, 2, 3, 4, 6)  # of the motion floats


# ---------------------------------------------------------------- label volumes
def label_values(K):
    """K distinct label values in the int16 range, a negative one and the extremes among them when K allows"""
    base = [10, -7, 32767, -32768, 49]
    return (base + [100 + 3 * i for i in range(K)])[:K]


def label_volume(recipe, shape, labels, seed, block=4):
    """(D,H,W) int16 over the listed labels plus 0, a negative value and one unlisted label (0, -3 and 9999: in no list of
    label_values).  'blocks': a coarse random grid upsampled by nearest neighbour, `block` voxels
    per cell (spatially coherent, like anatomy); 'white':
    independent draws per voxel"""
    rng = np.random.default_rng(seed)
    values = np.array(list(labels) + [0, -3, 9999], dtype=np.int16)
    if recipe == 'white':
        return values[rng.integers(len(values), size=shape)]
    if recipe == 'blocks':
        g = [max(1, (n + block - 1) // block) for n in shape]
        coarse = values[rng.integers(len(values), size=g)]
        idx = [np.minimum(np.arange(n) // block, gn - 1) for n, gn in zip(shape, g)]
        return coarse[np.ix_(*idx)]
    raise ValueError(recipe)


LABEL_RECIPES = ('blocks', 'white')


def structure_index_np(seg, labels, mask=None):
    """(V,) int64: the structure of every voxel, -1 for none"""
    seg = np.asarray(seg).reshape(-1).astype(np.int64)
    idx = np.full(seg.shape, -1, dtype=np.int64)
    for j, v in enumerate(labels):
        idx[seg == int(v)] = j
    if mask is not None:
        idx[~(np.asarray(mask).reshape(-1) != 0)] = -1
    return idx


def _groups(idx, K):
    order = np.argsort(idx, kind='stable')
    bounds = np.searchsorted(idx[order], np.arange(K + 1))
    return [order[bounds[j]:bounds[j + 1]] for j in range(K)]


def _sum(x):
    return float(np.asarray(x, dtype=np.longdouble).sum())


# ---------------------------------------------------------------- the two reductions
def motion_np(displacement, transformation, seg, labels, scale=(1.0, 1.0, 1.0), mask=None, ref=None):
    """displacement, transformation (C,3,D,H,W) float32 -> dict: ints (C,K,2) int64, floats (C,K,9) float64 and, per (chain,
    structure), what the tolerances need: 'abs' (C,K,9) sum |term| of the sum columns, 'e_sum', 'e_max' (C,K), 'fold_lo',
    'fold_hi' (C,K).  ref: jacobian_posterior_np(transformation), if the caller has it"""
    u = np.asarray(displacement, dtype=np.float32).astype(np.float64)
    Cn = u.shape[0]
    K = len(labels)
    ref = jacobian_posterior_np(np.asarray(transformation, dtype=np.float32)) if ref is None else ref
    det, e = ref['det'].reshape(Cn, -1), ref['e'].reshape(Cn, -1)
    groups = _groups(structure_index_np(seg, labels, mask), K)
    s = np.asarray(scale, dtype=np.float32).astype(np.float64)
    w = u.reshape(Cn, 3, -1) * s.reshape(1, 3, 1)  # exact
    n2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    n1 = np.sqrt(n2)
    ints = np.zeros((Cn, K, MOTION_INTS), dtype=np.int64)
    floats = np.zeros((Cn, K, MOTION_FLOATS), dtype=np.float64)
    floats[:, :, (5, 8)] = -np.inf
    floats[:, :, 7] = np.inf
    absum = np.zeros((Cn, K, MOTION_FLOATS))
    e_sum, e_max = np.zeros((Cn, K)), np.zeros((Cn, K))
    fold_lo, fold_hi = np.zeros((Cn, K), dtype=np.int64), np.zeros((Cn, K), dtype=np.int64)
    for c in range(Cn):
        for j, g in enumerate(groups):
            if g.size == 0:
                continue
            d = det[c, g]
            ok = ~np.isnan(d)
            terms = [w[c, 0, g], w[c, 1, g], w[c, 2, g], n1[c, g], n2[c, g], None, d[ok]]
            ints[c, j] = (g.size, int((~(d > 0)).sum()))
            for col in SUM_COLUMNS:
                floats[c, j, col] = _sum(terms[col])
                absum[c, j, col] = _sum(np.abs(terms[col]))
            floats[c, j, 5] = np.fmax.reduce(n1[c, g], initial=-np.inf)
            if ok.any():
                floats[c, j, 7], floats[c, j, 8] = d[ok].min(), d[ok].max()
                e_sum[c, j], e_max[c, j] = _sum(e[c, g][ok]), e[c, g][ok].max()
            nan = ~ok
            fold_lo[c, j] = int(((d <= -DELTA) | nan).sum())
            fold_hi[c, j] = int(((d < DELTA) | nan).sum())
    return {'ints': ints, 'floats': floats, 'abs': absum, 'e_sum': e_sum, 'e_max': e_max, 'fold_lo': fold_lo, 'fold_hi': fold_hi}


def motion_errors(got_ints, got_floats, want):
    """-> (the largest error / tolerance over every float column, a list of the violations): the comparison of the module
    docstring; where the restatement holds the identity of an empty structure (or of one whose det J are all NaN), the same
    value is asked for"""
    with np.errstate(invalid='ignore'):  # inf - inf, where both sides hold such an identity
        return _motion_errors(got_ints, got_floats, want)


def _motion_errors(got_ints, got_floats, want):
    gi, gf = np.asarray(got_ints), np.asarray(got_floats)
    wi, wf = want['ints'], want['floats']
    bad, worst = [], 0.0
    if not np.array_equal(gi[..., 0], wi[..., 0]):
        bad.append('voxels')
    if not ((want['fold_lo'] <= gi[..., 1]) & (gi[..., 1] <= want['fold_hi'])).all():
        bad.append('folded')
    m = wi[..., 0].astype(np.float64)
    for col in SUM_COLUMNS:
        tol = m * EPS * want['abs'][..., col] + (FACTOR * want['e_sum'] if col == 6 else 0.0)
        err = np.abs(gf[..., col] - wf[..., col])
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(err == 0, 0.0, err / tol)
        worst = max(worst, float(np.nanmax(ratio)))
        if not (err <= tol).all():
            bad.append(f'column {col}')
    has = np.isfinite(wf[..., 5])
    if not np.array_equal(gf[..., 5][~has], wf[..., 5][~has]) or not (np.abs(gf[..., 5] - wf[..., 5])[has] <= 2 * np.spacing(wf[..., 5][has])).all():
        bad.append('max |w|')
    for col in (7, 8):
        has = np.isfinite(wf[..., col])
        if not np.array_equal(gf[..., col][~has], wf[..., col][~has]) or not (np.abs(gf[..., col] - wf[..., col])[has] <= want['e_max'][has]).all():
            bad.append(f'column {col}')
        if has.any():
            with np.errstate(invalid='ignore', divide='ignore'):
                r = np.abs(gf[..., col] - wf[..., col])[has] / want['e_max'][has]
            worst = max(worst, float(np.nanmax(np.where(np.isnan(r), 0.0, r))))
    return worst, bad


def map_stats_np(maps, seg, labels, mask=None):
    """maps (M,D,H,W) float32 -> dict: ints (M,K,2), floats (M,K,4), 'abs' (M,K,2): sum |x|, sum x^2"""
    maps = np.asarray(maps, dtype=np.float32)
    M, K = maps.shape[0], len(labels)
    groups = _groups(structure_index_np(seg, labels, mask), K)
    ints = np.zeros((M, K, MAP_INTS), dtype=np.int64)
    floats = np.zeros((M, K, MAP_FLOATS), dtype=np.float64)
    floats[:, :, 2], floats[:, :, 3] = np.inf, -np.inf
    absum = np.zeros((M, K, 2))
    flat = maps.reshape(M, -1).astype(np.float64)
    for m in range(M):
        for j, g in enumerate(groups):
            x = flat[m, g]
            fin = np.isfinite(x)
            ints[m, j] = (int(fin.sum()), int((~fin).sum()))
            x = x[fin]
            if x.size:
                floats[m, j] = (_sum(x), _sum(x * x), x.min(), x.max())
                absum[m, j] = (_sum(np.abs(x)), _sum(x * x))
    return {'ints': ints, 'floats': floats, 'abs': absum}


def map_errors(got_ints, got_floats, want):
    gi, gf = np.asarray(got_ints), np.asarray(got_floats)
    bad, worst = [], 0.0
    if not np.array_equal(gi, want['ints']):
        bad.append('counts')
    m = want['ints'][..., 0].astype(np.float64)
    for col in (0, 1):
        tol = m * EPS * want['abs'][..., col]
        err = np.abs(gf[..., col] - want['floats'][..., col])
        with np.errstate(invalid='ignore', divide='ignore'):
            worst = max(worst, float(np.nanmax(np.where(err == 0, 0.0, err / tol))))
        if not (err <= tol).all():
            bad.append(f'column {col}')
    if not np.array_equal(gf[..., 2:], want['floats'][..., 2:]):
        bad.append('min / max')
    return worst, bad


# ---------------------------------------------------------------- the host summary
def split_rhat_np(series):
    """(C, N) -> scalar split R-hat (BDA3 section 11.4): halves of N // 2, sqrt(((h - 1) / h W + B) / W)"""
    C, N = series.shape
    h = N // 2
    halves = np.concatenate([series[:, :h], series[:, N - h:]], axis=0)
    means = halves.mean(axis=1)
    W = float(np.mean(halves.var(axis=1, ddof=1)))
    B = float(means.var(ddof=1))
    if W == 0.0:
        return 1.0 if B == 0.0 else math.inf
    return math.sqrt(((h - 1) / h * W + B) / W)


def summary_np(ints, floats, names, spacing=(1.0, 1.0, 1.0), chains=1, cov_trace=None):
    """the per-structure table of structure_report.structure_summary, written out again from its definitions"""
    ints, floats = np.asarray(ints).astype(np.int64), np.asarray(floats).astype(np.float64)
    n, K = ints.shape[:2]
    chain = np.arange(n) % chains
    out = {}
    for j, name in enumerate(names):
        vox = int(ints[0, j, 0])
        row = {'voxels': vox}
        keys = ('shift_mean_x', 'shift_mean_y', 'shift_mean_z', 'shift_mean_norm', 'shift_std_major', 'shift_std_minor',
                'shift_std_total', 'disp_mean', 'disp_rms', 'disp_max', 'vol_ratio_mean', 'vol_ratio_std', 'vol_mean_mm3', 'fold_frac',
                'det_min', 'det_max', 'rhat_max') + (('coherence', 'n_eff') if cov_trace is not None else ())
        row.update(dict.fromkeys(keys, math.nan))
        out[name] = row
        if vox == 0:
            continue
        s = floats[:, j, 0:3] / vox
        mean = s.mean(axis=0)
        row['shift_mean_x'], row['shift_mean_y'], row['shift_mean_z'] = mean.tolist()
        row['shift_mean_norm'] = float(np.linalg.norm(mean))
        ratio = floats[:, j, 6] / vox
        if n >= 2:
            cov = np.cov(s.T, ddof=1)
            w = np.linalg.eigvalsh(cov)
            row['shift_std_major'], row['shift_std_minor'] = math.sqrt(max(w[-1], 0.0)), math.sqrt(max(w[0], 0.0))
            row['shift_std_total'] = math.sqrt(max(np.trace(cov), 0.0))
            row['vol_ratio_std'] = float(ratio.std(ddof=1))
        row['disp_mean'] = float((floats[:, j, 3] / vox).mean())
        row['disp_rms'] = math.sqrt(float((floats[:, j, 4] / vox).mean()))
        row['disp_max'] = float(floats[:, j, 5].max())
        row['vol_ratio_mean'] = float(ratio.mean())
        row['vol_mean_mm3'] = row['vol_ratio_mean'] * vox * float(np.prod(spacing))
        row['fold_frac'] = float((ints[:, j, 1] / vox).mean())
        row['det_min'], row['det_max'] = float(floats[:, j, 7].min()), float(floats[:, j, 8].max())
        per_chain = [int((chain == c).sum()) for c in range(chains)]
        if chains >= 2 and min(per_chain) >= 4:
            N = min(per_chain)
            row['rhat_max'] = max(split_rhat_np(np.stack([x[chain == c][:N] for c in range(chains)]))
                                  for x in (s[:, 0], s[:, 1], s[:, 2], ratio))
        if cov_trace is not None and n >= 2:
            row['coherence'] = float(np.trace(np.cov(s.T, ddof=1)) / cov_trace[j])
            row['n_eff'] = 1.0 / row['coherence']
    return out


def covariance_trace_np(records, seg, labels, scale=(1.0, 1.0, 1.0), mask=None):
    """records (n,3,D,H,W) -> (K,): the mean over each structure's voxels of trace Cov(u(x)), divisor n - 1, float64"""
    u = np.asarray(records, dtype=np.float64)
    n = u.shape[0]
    var = u.var(axis=0, ddof=1).reshape(3, -1) * (np.asarray(scale, dtype=np.float64).reshape(3, 1) ** 2)
    groups = _groups(structure_index_np(seg, labels, mask), len(labels))
    return np.array([var[:, g].sum(axis=0).mean() if g.size and n >= 2 else np.nan for g in groups])
