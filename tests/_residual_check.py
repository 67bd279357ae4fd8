"""numpy restatement of the residual model check (include/irsgmcmc.h: irs_residual_*; ir_sgmcmc_amd/residual_check.py).

It shares no code with the HIP path or with residual_check.py: the binning repeats the float32 operations of the definition one
by one, the sums are exact (math.fsum over float64), the fit is written out from its formulas with plain loops, and the NLL
recursion runs in float64 -- what the float32 recursion of the kernel approximates."""
import math

import numpy as np

f32 = np.float32
COUNTS = ('n', 'n_nonfinite', 'n_clipped')
FIT_KEYS = ('kl', 'tv', 'ks', 'chi2', 'tail', 'tail_model', 'mean', 'std', 'std_model', 'kurtosis', 'kurtosis_model', 'n')


# ---------------------------------------------------------------- generators
def draw_mixture(shape, C, std, proportions, seed):
    """(C,1,*shape) float32 draws from the zero-mean mixture"""
    rng = np.random.default_rng(seed)
    n = C * int(np.prod(shape))
    k = rng.choice(len(std), size=n, p=np.asarray(proportions, np.float64) / np.sum(proportions))
    return (rng.standard_normal(n) * np.asarray(std, np.float64)[k]).astype(f32).reshape(C, 1, *shape)


def flat_background(shape, C, std, proportions, seed):
    """mixture draws that are exactly 0 on the first half of every chain's voxels: whole wavefronts in one bin"""
    z = draw_mixture(shape, C, std, proportions, seed)
    flat = z.reshape(C, -1)
    flat[:, :(flat.shape[1] + 1) // 2] = 0.0
    return z


def random_mask(shape, seed, dtype=bool):
    rng = np.random.default_rng(seed)
    return (rng.random((1, 1, *shape)) < 0.6).astype(dtype)


def spoil(z, mask, half_range, seed):
    """NaN, +inf, -inf and |z| > half_range (both signs, one far beyond the int range once binned) planted inside and outside
    the mask (anywhere when it is None); -> a copy"""
    z = z.copy()
    rng = np.random.default_rng(seed)
    C, V = z.shape[0], int(np.prod(z.shape[2:]))
    inside = np.arange(V) if mask is None else np.flatnonzero(mask.reshape(-1))
    outside = np.zeros(0, int) if mask is None else np.flatnonzero(mask.reshape(-1) == 0)
    bad = [np.nan, np.inf, -np.inf, 1.5 * half_range, -2.0 * half_range, 3e38, -1e30, np.nextafter(f32(half_range), f32(np.inf))]
    for c in range(C):
        flat = z[c].reshape(-1)
        for where in (inside, outside):
            if len(where) >= 2 * len(bad):
                pick = rng.choice(where, size=2 * len(bad), replace=False)
                flat[pick] = np.asarray(bad + bad, f32)
    return z


# ---------------------------------------------------------------- histogram, counts, sums
def bin_index(z, half_range, bins):
    """the bin of every float32 z, each operation rounded to float32 as the definition states it; NaN gives bin 0"""
    h = f32(half_range)
    inv_w = f32(bins) / (f32(2.0) * h)
    with np.errstate(over='ignore', invalid='ignore'):
        t = np.floor((z.astype(f32) + h) * inv_w)
    t = np.where(np.isnan(t), f32(0.0), t)
    return np.minimum(np.maximum(t, f32(0.0)), f32(bins - 1)).astype(np.int64)


def reference_histogram(z, mask, half_range, bins):
    """z (C,1,D,H,W) float32, mask (1,1,D,H,W) or None -> hist (C,bins) int64, counts (C,3) int64, sums (C,4) float64"""
    C = z.shape[0]
    hist, counts, sums = np.zeros((C, bins), np.int64), np.zeros((C, 3), np.int64), np.zeros((C, 4), np.float64)
    m = np.ones(z[0].size, bool) if mask is None else mask.reshape(-1) != 0
    for c in range(C):
        zc = z[c].reshape(-1)
        finite = np.isfinite(zc)
        take = m & finite
        zt = zc[take]
        hist[c] = np.bincount(bin_index(zt, half_range, bins), minlength=bins)
        counts[c] = [take.sum(), (m & ~finite).sum(), (np.abs(zt) > f32(half_range)).sum()]
        d = zt.astype(np.float64)
        sums[c] = [math.fsum(d), math.fsum(d * d), math.fsum((d * d) ** 2), np.abs(d).max() if d.size else -np.inf]
    return hist, counts, sums


def accumulate(state, new):
    """what a later call adds to the state of the earlier ones"""
    (h0, c0, s0), (h1, c1, s1) = state, new
    s = s0 + s1
    s[:, 3] = np.maximum(s0[:, 3], s1[:, 3])
    return h0 + h1, c0 + c1, s


# ---------------------------------------------------------------- fit
def cdf(x, std, proportions):
    total = 0.0
    for s, p in zip(std, proportions):
        total += p * 0.5 * math.erfc(-x / (s * math.sqrt(2.0)))
    return total


def reference_fit(hist, counts, sums, half_range, std, proportions):
    """one chain: hist (B,), counts (3,), sums (4,) -> the dict of FIT_KEYS"""
    B, n, h = len(hist), int(counts[0]), float(half_range)
    if n == 0:
        return {**{k: math.nan for k in FIT_KEYS}, 'n': 0}
    edge = [-h + 2.0 * h * b / B for b in range(B + 1)]
    p = []
    for b in range(B):
        if b == 0:
            p.append(cdf(edge[1], std, proportions))
        elif b == B - 1:
            p.append(0.5 * sum(pk * math.erfc(edge[B - 1] / (s * math.sqrt(2.0))) for s, pk in zip(std, proportions)))
        else:
            p.append(cdf(edge[b + 1], std, proportions) - cdf(edge[b], std, proportions))
    q = [int(x) / n for x in hist]
    kl = 0.0
    for qb, pb in zip(q, p):
        if qb > 0:
            kl = math.inf if pb == 0 else kl + qb * math.log(qb / pb)
    ks, run = 0.0, 0.0
    for b in range(1, B):
        run += q[b - 1]
        ks = max(ks, abs(run - cdf(edge[b], std, proportions)))
    s1, s2, s4 = float(sums[0]), float(sums[1]), float(sums[2])
    var = sum(pk * s * s for s, pk in zip(std, proportions))
    return {'kl': kl, 'tv': 0.5 * sum(abs(qb - pb) for qb, pb in zip(q, p)), 'ks': ks,
            'chi2': sum((qb - pb) ** 2 / pb for qb, pb in zip(q, p) if pb > 0), 'tail': int(counts[2]) / n,
            'tail_model': sum(pk * math.erfc(h / (s * math.sqrt(2.0))) for s, pk in zip(std, proportions)),
            'mean': s1 / n, 'std': math.sqrt(s2 / n), 'std_model': math.sqrt(var),
            'kurtosis': n * s4 / (s2 * s2) if s2 > 0 else math.nan,
            'kurtosis_model': 3.0 * sum(pk * s ** 4 for s, pk in zip(std, proportions)) / var ** 2, 'n': n}


# ---------------------------------------------------------------- the NLL map
def mixture_terms(std, proportions):
    """(log_weight, inv_std) float64 arrays"""
    std, pi = np.asarray(std, np.float64), np.asarray(proportions, np.float64)
    return np.log(pi) - np.log(std) - 0.5 * math.log(2.0 * math.pi), 1.0 / std


def nll(z, log_weight, inv_std):
    """-log sum_k exp(log_weight_k - (z inv_std_k)^2 / 2) in float64, by the maximum; z any shape, finite"""
    a = np.asarray(log_weight)[:, None] - 0.5 * (z.reshape(1, -1).astype(np.float64) * np.asarray(inv_std)[:, None]) ** 2
    m = a.max(axis=0)
    return (-(m + np.log(np.exp(a - m).sum(axis=0)))).reshape(z.shape)


def reference_nll_map(records, models):
    """records: list of (C,1,D,H,W) float32; models: one (log_weight, inv_std) per record -> mean (D,H,W) float64 -- the true
    running mean of the float64 NLL over the finite samples --, count (D,H,W) int32, and the largest |nll| that entered"""
    shape = records[0].shape[2:]
    mean, count, biggest = np.zeros(shape, np.float64), np.zeros(shape, np.int32), 0.0
    for z, (lw, inv) in zip(records, models):
        for c in range(z.shape[0]):
            ok = np.isfinite(z[c, 0])
            x = nll(z[c, 0][ok], lw, inv)
            count[ok] += 1
            mean[ok] += (x - mean[ok]) / count[ok]
            biggest = max(biggest, float(np.abs(x).max()) if x.size else 0.0)
    return mean, count, biggest


def reference_nll_summary(mean, count, mask):
    """isummary {voxels, voxels with count == 0}, fsummary {sum of mean, max of mean} over the mask (None: everything); mean as
    the float32 map the kernel reads"""
    m = np.ones(mean.shape, bool) if mask is None else mask.reshape(mean.shape) != 0
    some = m & (count > 0)
    vals = mean[some].astype(np.float64)
    return [int(m.sum()), int((m & (count == 0)).sum())], [math.fsum(vals), float(vals.max()) if vals.size else -math.inf]
