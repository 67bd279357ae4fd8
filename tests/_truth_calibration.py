"""numpy restatement of the known-transformation validation (include/irsgmcmc.h: irs_truth_update, irs_truth_calibrate;
ir_sgmcmc_amd/truth.py: simulate_velocity, calibration_summary): the same operations in the same order in float64 -- numpy
rounds every operation once and contracts nothing, as the kernels do -- so that maps, counts and maxima are compared bit for bit
and sums under the bound of a reordered sum.  Shared by the host and the GPU tests."""
import math

import numpy as np


def velocity_np(dims, seed, amplitude, modes=6, max_wavenumber=2):
    """simulate_velocity restated"""
    dims = tuple(dims)
    rng = np.random.default_rng(seed)
    k = rng.integers(1, max_wavenumber + 1, size=(3, modes, 3))
    phase = rng.uniform(0.0, 2.0 * np.pi, size=(3, modes, 3))
    weight = rng.standard_normal((3, modes))
    z, y, x = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in dims], indexing='ij')
    xi = (z, y, x)
    v = np.zeros((3,) + dims)
    for c in range(3):
        for m in range(modes):
            term = np.full(dims, weight[c, m])
            for a in range(3):
                term = term * np.sin(np.pi * k[c, m, a] * xi[a] + phase[c, m, a])
            v[c] += term
        v[c] *= ((1.0 - z ** 2) * (1.0 - y ** 2)) * (1.0 - x ** 2)
    peak = np.abs(v).max()
    if amplitude == 0 or not peak > 0:
        return np.zeros((3,) + dims, dtype=np.float32)
    a32 = np.float32(amplitude)
    out = np.clip((v * (amplitude / peak)).astype(np.float32), -a32, a32)
    at = np.unravel_index(int(np.argmax(np.abs(v))), v.shape)
    out[at] = a32 if v[at] > 0 else -a32
    return out


def update_np(u, t, below, records_before, scale=(1.0, 1.0, 1.0), mask=None):
    """u (C,3,D,H,W), t (3,D,H,W) float32; below (3,D,H,W) uint16 or None -> (below after, ints (C,2) int64, floats (C,3) float64,
    bound (C,2): N * 2^-53 * sum |term| of the two sums).  records_before = 0 ignores `below`."""
    u, t = np.asarray(u, dtype=np.float32), np.asarray(t, dtype=np.float32)
    C = u.shape[0]
    start = np.zeros(t.shape, dtype=np.int64) if records_before == 0 else np.asarray(below).astype(np.int64)
    with np.errstate(invalid='ignore'):
        new = start + (u < t[None]).sum(axis=0)
    m = np.ones(t.shape[1:], dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    s = np.asarray(scale, dtype=np.float32).astype(np.float64).reshape(3, 1)
    ints, floats, bound = np.zeros((C, 2), dtype=np.int64), np.zeros((C, 3)), np.zeros((C, 2))
    with np.errstate(all='ignore'):
        for c in range(C):
            e = s * (u[c][:, m].astype(np.float64) - t[:, m].astype(np.float64))
            q = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            fin = np.isfinite(q)
            r = np.sqrt(q[fin])
            ints[c] = (q.size, int((~fin).sum()))
            floats[c] = (r.sum(), q[fin].sum(), r.max() if r.size else -np.inf)
            bound[c] = (q.size * 2.0 ** -53 * r.sum(), q.size * 2.0 ** -53 * q[fin].sum())
    return new.astype(np.uint16), ints, floats, bound


def calibrate_np(mean, comoment, below, t, n, scale, d2_edges, levels, rank_bins, var_edges, std_floor=1e-3, mask=None):
    """-> dict: 'error', 'mahalanobis' (D,H,W) float32; 'pit_hist' (B,), 'coverage' (L,), 'rank_hist' (3,Br) int64; 'rel_ints'
    (R,), 'rel_floats' (R,2); 'isummary' (3,), 'fsummary' (9,); 'fbound' (9,), 'rel_bound' (R,2): the reordered-sum bounds (0 for
    the maxima); 'd2', 'v', 'finite', 'raised' per voxel"""
    mu, M, t = (np.asarray(a, dtype=np.float32) for a in (mean, comoment, t))
    dims = mu.shape[1:]
    s = np.asarray(scale, dtype=np.float32).astype(np.float64)
    f2 = float(std_floor) * float(std_floor)
    nm1 = float(n - 1)
    with np.errstate(all='ignore'):
        fin = np.isfinite(mu).all(axis=0) & np.isfinite(M).all(axis=0) & np.isfinite(t).all(axis=0)
        dl = [s[c] * (mu[c].astype(np.float64) - t[c].astype(np.float64)) for c in range(3)]
        entry = lambda a, b, k: ((s[a] * s[b]) * M[k].astype(np.float64)) / nm1
        axx, ayy, azz = entry(0, 0, 0) + f2, entry(1, 1, 1) + f2, entry(2, 2, 2) + f2
        axy, axz, ayz = entry(0, 1, 3), entry(0, 2, 4), entry(1, 2, 5)
        raised = np.zeros(dims, dtype=bool)

        def pivot(d):
            low = ~(d >= f2)
            raised[...] |= low
            return np.where(low, f2, d)

        d0 = pivot(axx)
        l10, l20 = axy / d0, axz / d0
        d1 = pivot(ayy - l10 * axy)
        w = ayz - l20 * axy
        l21 = w / d1
        d2 = pivot((azz - l20 * axz) - l21 * w)
        y0 = dl[0]
        y1 = dl[1] - l10 * y0
        y2 = (dl[2] - l20 * y0) - l21 * y1
        dist2 = (y0 * y0 / d0 + y1 * y1 / d1) + y2 * y2 / d2
        e2 = [dl[c] * dl[c] for c in range(3)]
        err2 = (e2[0] + e2[1]) + e2[2]
        v = (axx + ayy) + azz
        z = [e2[0] / np.where(axx >= f2, axx, f2), e2[1] / np.where(ayy >= f2, ayy, f2), e2[2] / np.where(azz >= f2, azz, f2)]
        fin = fin & np.isfinite(dist2)
        err = np.sqrt(err2)
        error = np.where(fin, err, np.nan).astype(np.float32)
        mahalanobis = np.where(fin, np.sqrt(dist2), np.nan).astype(np.float32)
    m = np.ones(dims, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    take = m & fin
    d2_edges, levels, var_edges = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (d2_edges, levels, var_edges))
    B, R, Br = len(d2_edges) + 1, len(var_edges) + 1, int(rank_bins)
    dt, vt, et = dist2[take], v[take], err2[take]
    pit = np.bincount((d2_edges[None, :] <= dt[:, None]).sum(axis=1), minlength=B).astype(np.int64)
    coverage = np.asarray([(dt <= lv).sum() for lv in levels], dtype=np.int64)
    bl = np.asarray(below).astype(np.int64)
    rank = np.stack([np.bincount(np.minimum(bl[c][take] * Br // (n + 1), Br - 1), minlength=Br) for c in range(3)]).astype(np.int64)
    rbin = np.minimum((var_edges[None, :] <= vt[:, None]).sum(axis=1), R - 1)
    rel_ints = np.bincount(rbin, minlength=R).astype(np.int64)
    rel_floats = np.stack([np.bincount(rbin, weights=vt, minlength=R), np.bincount(rbin, weights=et, minlength=R)], axis=1)
    N = int(m.sum())
    eps = N * 2.0 ** -53
    rel_bound = eps * np.stack([np.bincount(rbin, weights=np.abs(vt), minlength=R), np.bincount(rbin, weights=et, minlength=R)], axis=1)
    errt = err[take]
    neg_inf = -np.inf
    fsummary = np.asarray([errt.sum(), et.sum(), errt.max() if errt.size else neg_inf, dt.sum(), dt.max() if dt.size else neg_inf,
                           vt.sum(), z[0][take].sum(), z[1][take].sum(), z[2][take].sum()])
    fbound = eps * np.asarray([errt.sum(), et.sum(), 0.0, np.abs(dt).sum(), 0.0, np.abs(vt).sum(), np.abs(z[0][take]).sum(),
                               np.abs(z[1][take]).sum(), np.abs(z[2][take]).sum()])
    isummary = np.asarray([N, int((m & ~fin).sum()), int((take & raised).sum())], dtype=np.int64)
    return {'error': error, 'mahalanobis': mahalanobis, 'pit_hist': pit, 'coverage': coverage, 'rank_hist': rank, 'rel_ints': rel_ints,
            'rel_floats': rel_floats, 'isummary': isummary, 'fsummary': fsummary, 'fbound': fbound, 'rel_bound': rel_bound,
            'd2': dist2, 'v': v, 'finite': fin, 'raised': raised}


def welford_np(records):
    """records (n,3,D,H,W) float32 -> (mean (3,...), comoment (6,...: xx, yy, zz, xy, xz, yz)) float32, the float32 recurrence of
    irs_displacement_covariance_update: delta = x - mean; mean += delta / k; comoment_ab += delta_a * (x_b - mean_b)"""
    x = np.asarray(records, dtype=np.float32)
    mean = np.zeros(x.shape[1:], dtype=np.float32)
    M = np.zeros((6,) + x.shape[2:], dtype=np.float32)
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    with np.errstate(all='ignore'):
        for k, r in enumerate(x, start=1):
            if k == 1:
                mean, M = r.copy(), np.zeros_like(M)
                continue
            delta = r - mean
            mean = mean + delta / np.float32(k)
            for j, (a, b) in enumerate(pairs):
                M[j] = M[j] + delta[a] * (r[b] - mean[b])
    return mean, M


def rank_fractions_np(n, Br):
    """the exact probability of every rank bin when the rank is uniform on 0 .. n, by counting"""
    out = np.zeros(Br)
    for r in range(n + 1):
        out[r * Br // (n + 1)] += 1.0
    return out / (n + 1)


def summary_np(res, n, levels, reference='hotelling'):
    """the derived numbers the tests compare with truth.calibration_summary: coverage fractions, chi^2 of the rank histograms
    against the exact expectation, scale factor"""
    voxels, nonfinite, _ = (int(v) for v in res['isummary'])
    finite = voxels - nonfinite
    frac = rank_fractions_np(n, res['rank_hist'].shape[1])
    expected = math.sqrt((1.0 + 1.0 / n) * (n - 1.0) / (n - 5.0)) if reference == 'hotelling' else 1.0
    pit = res['pit_hist']
    B = len(pit)
    return {'coverage': [int(c) / finite for c in res['coverage']],
            'rank_chi2': [float((((res['rank_hist'][c] - frac * finite) ** 2) / (frac * finite)).sum()) for c in range(3)],
            'scale_factor': math.sqrt(res['fsummary'][3] / (3.0 * finite)) / expected,
            'pit_chi2': float(((pit - finite / B) ** 2 / (finite / B)).sum()),
            'rmse': math.sqrt(res['fsummary'][1] / finite), 'mean': res['fsummary'][0] / finite, 'max': res['fsummary'][2]}


def gaussian_case(dims=(12, 10, 14), n=63, seed=20261020, truth_factor=1.0):
    """The case with a known answer: per voxel a random SPD Sigma_x, n iid N(0, Sigma_x) records and a truth drawn from the same
    law (times truth_factor) -> (records (n,3,D,H,W) float32, truth (3,D,H,W) float32)"""
    rng = np.random.default_rng(seed)
    V = int(np.prod(dims))
    A = rng.standard_normal((V, 3, 3))
    Sigma = A @ A.transpose(0, 2, 1) + 0.1 * np.eye(3)
    Lc = np.linalg.cholesky(Sigma)
    rec = np.einsum('vab,nvb->nva', Lc, rng.standard_normal((n, V, 3)))
    truth = truth_factor * np.einsum('vab,vb->va', Lc, rng.standard_normal((V, 3)))
    to_grid = lambda a: np.ascontiguousarray(np.moveaxis(a.reshape(a.shape[:-2] + tuple(dims) + (3,)), -1, -4)).astype(np.float32)
    return to_grid(rec), to_grid(truth)
