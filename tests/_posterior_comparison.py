"""numpy restatement of the posterior comparison ("Posterior comparison"), the case generators, the
tolerances and the checks, shared by the host and GPU tests.

The restatement evaluates the definitions in float64 from a given pair of float32 states: S_X = diag(s) M_X diag(s) / (n_X - 1),
Delta = s o (mu_A - mu_B), the eigen-decompositions by numpy.linalg.eigh (the device runs cyclic Jacobi sweeps: an independent
solver), eigenvalues clamped at 0.  R = S_B^1/2 S_A S_B^1/2 is formed from the full matrix square root and symmetrised before
numpy.linalg.eigvalsh.  The two traces of the Jeffreys divergence are summed over the overlaps of the two eigenbases,
tr(B~^-1 A~) = sum_ik (e^B_i . e^A_k)^2 fa_k / fb_i, as the device sums them: the two sides differ only in their eigen-solver.

Tolerances.  Everything is measured against this restatement evaluated on the device's own float32 states.
  shift, log_std_ratio   a handful of double operations: the restatement rounded to float32, +-1 float32 ulp.
  bures                  compared as squares: |bures^2 - want^2| <= C_B 2^-26 (tr S_A + tr S_B) + 2^-22 want^2.  The square root of
                         an eigenvalue of R near zero is not Lipschitz: two correct float64 evaluations differ by about
                         sqrt(2^-53) tr, not 2^-53 tr.  The second term is the float32 storage, squared back.
  jeffreys               |jeffreys - want| <= C_J 2^-53 T + 2^-23 |want|, T the sum of the absolute values of its terms,
                         1/2 [tr(B~^-1 A~) + tr(A~^-1 B~) + 6 + Delta^T (A~^-1 + B~^-1) Delta], the floored inverses included.

C_B and C_J are four times the worst ratio, in units of the forms above with c = 1, between the host build of compare_device.h
(tests/csrc/compare_check.cpp eval) and this restatement over the cases of this module -- the known answers, the identical
states and every random case, states accumulated in float32 numpy.  The factor covers the device's fused multiply-adds.
Measured on the CPU (test_posterior_comparison_host.py prints them; it asserts that the host build stays inside the tolerances):
  bures     worst ratio 0.879 (rank-one records under the scale (1.5, 0.25, 40))  ->  MEASURED_B = 0.88, C_B = 3.52
  jeffreys  worst ratio 14.0 (identical anisotropic states of 4 records, where the answer is 0 and the storage term with it;
            every pair of different states stays inside the storage term alone)     ->  MEASURED_J = 14, C_J = 56
shift and log_std_ratio of the host build equal the rounded restatement bit for bit in every case.
"""
import numpy as np

from tests._displacement_covariance import case_mask, default_scale, draw_records, matrices, welford_np

MEASURED_B, MEASURED_J = 0.88, 14.0
C_B, C_J = 4 * MEASURED_B, 4 * MEASURED_J
STD_FLOOR = 1e-3
PLANES = ('shift', 'log_std_ratio', 'bures', 'jeffreys')
INT_KEYS = ('records_vi', 'records_mcmc', 'voxels', 'nonfinite_voxels', 'floored_voxels')
FLOAT_KEYS = ('shift_mean', 'shift_max', 'log_std_ratio_mean', 'log_std_ratio_min', 'log_std_ratio_max', 'std_ratio',
              'frac_vi_narrower', 'bures_mean', 'bures_max', 'w2_mean', 'w2_max', 'jeffreys_mean', 'jeffreys_max', 'std_total_vi',
              'std_total_mcmc')


def compare_np(mean_a, M_a, n_a, mean_b, M_b, n_b, scale, std_floor=STD_FLOOR):
    """the float64 restatement from two states (mean (3,...), M (6,...), whatever precision they were accumulated in) -> dict:
    the four planes (float64, NaN where a state value is not finite), bures2, terms (T of the module docstring), tr_a, tr_b,
    finite, floored"""
    mean_a, M_a, mean_b, M_b = (np.asarray(x) for x in (mean_a, M_a, mean_b, M_b))
    finite = np.isfinite(mean_a).all(axis=0) & np.isfinite(M_a).all(axis=0) & np.isfinite(mean_b).all(axis=0) & np.isfinite(M_b).all(axis=0)
    scale = np.asarray(scale, dtype=np.float64)
    f2 = float(std_floor) ** 2
    SA = matrices(np.where(finite, M_a, 0.0), n_a, scale)
    SB = matrices(np.where(finite, M_b, 0.0), n_b, scale)
    d = np.moveaxis(np.where(finite, mean_a.astype(np.float64) - mean_b.astype(np.float64), 0.0), 0, -1) * scale
    shift = np.sqrt((d ** 2).sum(axis=-1))
    tr_a, tr_b = np.trace(SA, axis1=-2, axis2=-1), np.trace(SB, axis1=-2, axis2=-1)
    ta, tb = np.maximum(tr_a, 3 * f2), np.maximum(tr_b, 3 * f2)
    big, small = np.maximum(ta, tb), np.minimum(ta, tb)
    log_std_ratio = np.where(ta >= tb, 0.5, -0.5) * np.log1p((big - small) / small)  # the device's form: see compare_device.h
    la, VA = np.linalg.eigh(SA)
    lb, VB = np.linalg.eigh(SB)
    la, lb = np.maximum(la, 0.0), np.maximum(lb, 0.0)
    floored = (la < f2).any(axis=-1) | (lb < f2).any(axis=-1)
    fa, fb = np.maximum(la, f2), np.maximum(lb, f2)
    # Bures: the full matrices
    root_b = np.einsum('...ik,...k,...jk->...ij', VB, np.sqrt(lb), VB)
    psd_a = np.einsum('...ik,...k,...jk->...ij', VA, la, VA)
    R = root_b @ psd_a @ root_b
    R = 0.5 * (R + np.swapaxes(R, -1, -2))
    lr = np.maximum(np.linalg.eigvalsh(R), 0.0)
    bures2 = np.maximum(tr_a + tr_b - 2.0 * np.sqrt(lr).sum(axis=-1), 0.0)
    # Jeffreys over the overlaps
    G2 = np.einsum('...ji,...jk->...ik', VB, VA) ** 2  # (e^B_i . e^A_k)^2
    tr = (G2 * (fa[..., None, :] / fb[..., :, None] + fb[..., :, None] / fa[..., None, :])).sum(axis=(-1, -2))
    pa, pb = np.einsum('...ji,...j->...i', VA, d), np.einsum('...ji,...j->...i', VB, d)
    quad = (pa ** 2 / fa + pb ** 2 / fb).sum(axis=-1)
    jeffreys = 0.5 * (tr - 6.0 + quad)
    nan = np.nan
    return {'shift': np.where(finite, shift, nan), 'log_std_ratio': np.where(finite, log_std_ratio, nan),
            'bures': np.where(finite, np.sqrt(bures2), nan), 'jeffreys': np.where(finite, jeffreys, nan),
            'bures2': bures2, 'terms': 0.5 * (tr + 6.0 + quad), 'tr_a': tr_a, 'tr_b': tr_b, 'finite': finite, 'floored': floored}


def ratios(ref, planes):
    """the stored float32 planes (dict of PLANES) against the restatement `ref` at its finite voxels -> name -> (worst error,
    worst ratio).  shift, log_std_ratio: the ratio is the error in float32 ulps of the rounded restatement.  bures (as squares),
    jeffreys: what the error exceeds the storage term by, in units of the bound form with c = 1 -- a ratio r meets the bound
    exactly when r <= C"""
    fin = ref['finite']
    out = {}
    for name in ('shift', 'log_std_ratio'):
        want = ref[name][fin].astype(np.float32)
        err = np.abs(planes[name][fin].astype(np.float64) - want.astype(np.float64))
        ulp = np.spacing(np.abs(want)).astype(np.float64)
        out[name] = (float(err.max()), float((err / ulp).max())) if err.size else (0.0, 0.0)
    got2, want2 = planes['bures'][fin].astype(np.float64) ** 2, ref['bures2'][fin]
    err = np.maximum(np.abs(got2 - want2) - 2.0 ** -22 * want2, 0.0)
    unit = 2.0 ** -26 * (ref['tr_a'][fin] + ref['tr_b'][fin])
    out['bures'] = _worst(err, unit)
    got, want = planes['jeffreys'][fin].astype(np.float64), ref['jeffreys'][fin]
    err = np.maximum(np.abs(got - want) - 2.0 ** -23 * np.abs(want), 0.0)
    out['jeffreys'] = _worst(err, 2.0 ** -53 * ref['terms'][fin])
    return out


def _worst(err, unit):
    if not err.size:
        return 0.0, 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err > 0, err / unit, 0.0)
    return float(err.max()), float(r.max())


def check_planes(ref, planes, label=''):
    """hold the stored float32 planes to the tolerances of the module docstring; prints the worst error and the worst error /
    tolerance per plane, then asserts.  -> the figures"""
    fin = ref['finite']
    for name in PLANES:
        p = np.asarray(planes[name])
        assert p.dtype == np.float32 and p.shape == fin.shape
        assert np.isnan(p[~fin]).all() and not np.isnan(p[fin]).any(), name
    r = ratios(ref, planes)
    figures = {'shift': r['shift'], 'log_std_ratio': r['log_std_ratio'], 'bures': (r['bures'][0], r['bures'][1] / C_B),
               'jeffreys': (r['jeffreys'][0], r['jeffreys'][1] / C_J)}
    print(label, {'voxels': int(fin.sum()), **figures})  # before the assertions
    for name in PLANES:
        assert figures[name][1] <= 1.0, (name, figures[name])
    return figures


def summary_np(planes, tr_a, tr_b, floored, n_a, n_b, mask=None):
    """the summary dict of posterior_comparison.comparison_summary over `mask`, from the given (stored) planes, the float64
    traces and the floored flags of the restatement"""
    p = {k: np.asarray(planes[k], dtype=np.float64) for k in PLANES}
    m = np.ones(p['shift'].shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    fin = m & ~np.isnan(p['shift'])
    voxels, k = int(m.sum()), int(fin.sum())
    out = {'records_vi': int(n_a), 'records_mcmc': int(n_b), 'voxels': voxels, 'nonfinite_voxels': voxels - k,
           'floored_voxels': int((np.asarray(floored) & fin).sum())}
    if k == 0:
        out.update(dict.fromkeys(FLOAT_KEYS, float('nan')))
        return out
    sh, lr, bu, je = (p[name][fin] for name in PLANES)
    w2 = np.sqrt(sh ** 2 + bu ** 2)
    out.update({'shift_mean': sh.sum() / k, 'shift_max': sh.max(), 'log_std_ratio_mean': lr.sum() / k, 'log_std_ratio_min': lr.min(),
                'log_std_ratio_max': lr.max(), 'std_ratio': np.exp(lr.sum() / k), 'frac_vi_narrower': (lr < 0).sum() / k,
                'bures_mean': bu.sum() / k, 'bures_max': bu.max(), 'w2_mean': w2.sum() / k, 'w2_max': w2.max(),
                'jeffreys_mean': je.sum() / k, 'jeffreys_max': je.max(), 'std_total_vi': np.sqrt(np.asarray(tr_a)[fin].sum() / k),
                'std_total_mcmc': np.sqrt(np.asarray(tr_b)[fin].sum() / k)})
    return {key: (v if key in INT_KEYS else float(v)) for key, v in out.items()}


def check_summary(summary, want):
    """integers exactly, floats to a 1e-6 relative difference (NaN where NaN is due)"""
    assert list(summary) == list(INT_KEYS[:2]) + list(INT_KEYS[2:]) + list(FLOAT_KEYS), list(summary)
    for key in INT_KEYS:
        assert summary[key] == want[key], (key, summary[key], want[key])
    for key in FLOAT_KEYS:
        g, w = summary[key], want[key]
        assert (np.isnan(g) and np.isnan(w)) or g == w or abs(g - w) <= 1e-6 * abs(w), (key, g, w)


# ---------------------------------------------------------------- known answers (scale 1, f = 1e-3, comoment = S (n - 1))
_R = np.sqrt(0.5)
_Q45 = np.array([[_R, -_R, 0.0], [_R, _R, 0.0], [0.0, 0.0, 1.0]])  # 45 degrees about the third axis
_DIAG = np.diag([4.0, 1.0, 0.25])
KNOWN = {  # name -> (S_A, mu_A, S_B, mu_B, shift, log_std_ratio, bures^2, jeffreys, floored)
    'diagonal': (_DIAG, (1.0, 2.0, 2.0), np.eye(3), (0.0, 0.0, 0.0), 3.0, 0.27980789396771, 1.25, 16.875, False),
    'rotated': (_Q45 @ _DIAG @ _Q45.T, (0.0, 0.0, 0.0), np.eye(3), (0.0, 0.0, 0.0), 0.0, 0.27980789396771, 1.25, 2.25, False),
    'rank one, orthogonal': (np.diag([4.0, 0.0, 0.0]), (0.0, 0.0, 0.0), np.diag([0.0, 9.0, 0.0]), (0.0, 0.0, 0.0), 0.0,
                             -0.40546510810816, 13.0, 6499998.0000002, True),
    'identical': (_Q45 @ np.diag([2.5, 0.7, 0.01]) @ _Q45.T, (0.3, -0.2, 0.1), _Q45 @ np.diag([2.5, 0.7, 0.01]) @ _Q45.T,
                  (0.3, -0.2, 0.1), 0.0, 0.0, 0.0, 0.0, False),
}
KNOWN_N = (5, 9)  # n_a, n_b of the known-answer states: comoment = S (n - 1) is exact in float32 for S of a few bits


def _six(S):
    return np.array([S[0, 0], S[1, 1], S[2, 2], S[0, 1], S[0, 2], S[1, 2]])


def known_states(shape=(4, 5, 6), seed=3):
    """float32 states over `shape` holding the four known cases, permuted across the voxels by a seeded permutation ->
    (mean_a (3,...), M_a (6,...), mean_b, M_b, which (...) int: the index into list(KNOWN) at every voxel)"""
    V = int(np.prod(shape))
    which = np.random.default_rng(seed).permutation(V) % len(KNOWN)
    names = list(KNOWN)
    out = [np.empty((c, V), dtype=np.float32) for c in (3, 6, 3, 6)]
    for v in range(V):
        SA, ma, SB, mb = KNOWN[names[which[v]]][:4]
        out[0][:, v], out[1][:, v] = ma, _six(SA) * (KNOWN_N[0] - 1)
        out[2][:, v], out[3][:, v] = mb, _six(SB) * (KNOWN_N[1] - 1)
    return tuple(x.reshape((-1,) + tuple(shape)) for x in out) + (which.reshape(shape),)


def check_known(planes, floored, which):
    """the planes (dict of PLANES, arrays over the known_states volume) against the table: shift and log_std_ratio to 1 float32
    ulp (exactly 0 where the answer is 0), bures^2 and jeffreys to the module's tolerances"""
    for idx, (name, row) in enumerate(KNOWN.items()):
        SA, _, SB, _, shift, lsr, b2, je, fl = row
        at = which == idx
        assert at.any()
        for key, want in (('shift', shift), ('log_std_ratio', lsr)):
            got = planes[key][at].astype(np.float64)
            w32 = np.float32(want)
            assert (np.abs(got - float(w32)) <= (float(np.spacing(np.abs(w32))) if want else 0.0)).all(), (name, key, got[0], want)
        tr = np.trace(SA) + np.trace(SB)
        err = np.abs(planes['bures'][at].astype(np.float64) ** 2 - b2)
        assert (err <= C_B * 2.0 ** -26 * tr + 2.0 ** -22 * b2).all(), (name, 'bures', err.max())
        terms = abs(je) + 6.0  # T = jeffreys + 6 where every term is positive
        err = np.abs(planes['jeffreys'][at].astype(np.float64) - je)
        assert (err <= C_J * 2.0 ** -53 * terms + 2.0 ** -23 * abs(je)).all(), (name, 'jeffreys', err.max())
        if floored is not None:
            assert (np.asarray(floored)[at] == fl).all(), (name, 'floored')


# ---------------------------------------------------------------- random cases
RECIPES = ('anisotropic', 'rank-one')
SHAPES = ((5, 7, 9), (8, 6, 10))  # V % 4 != 0 and == 0
RECORDS = ((4, 6), (40, 8))       # n_a (the VI side), n_b (the MCMC side)
OWN_SCALE = (1.5, 0.25, 40.0)


def draw_side(recipe, n, shape, seed):
    """n records (n,3,D,H,W) float32.  'anisotropic': draw_records' recipe.  'rank-one': draw_records' white noise about its
    mean field, projected at every voxel on one direction of a seeded field, so the sample covariance has rank one up to the
    float32 rounding of the records."""
    if recipe == 'anisotropic':
        return draw_records('anisotropic', n, shape, seed)
    if recipe != 'rank-one':
        raise ValueError(recipe)
    r = draw_records('white', n, shape, seed).astype(np.float64)
    u = np.random.default_rng(seed + 1).standard_normal((3,) + tuple(shape))
    u /= np.sqrt((u ** 2).sum(axis=0))
    m = r.mean(axis=0)
    along = ((r - m) * u).sum(axis=1, keepdims=True)
    return (m + along * u).astype(np.float32)


def case_seed(shape, n_a, n_b, recipe):
    return shape[2] * 100 + n_a + n_b + (5000 if recipe == 'rank-one' else 0)


def draw_pair(recipe, shape, n_a, n_b):
    seed = case_seed(shape, n_a, n_b, recipe)
    return draw_side(recipe, n_a, shape, seed), draw_side(recipe, n_b, shape, seed + 17)


def host_states(records_a, records_b):
    """the float32 states of the two sides by the Welford recurrences in float32 numpy (no fused multiply-add)"""
    ma, Ma = welford_np(records_a, np.float32)[:2]
    mb, Mb = welford_np(records_b, np.float32)[:2]
    return ma, Ma, mb, Mb


__all__ = ['C_B', 'C_J', 'MEASURED_B', 'MEASURED_J', 'STD_FLOOR', 'PLANES', 'INT_KEYS', 'FLOAT_KEYS', 'KNOWN', 'KNOWN_N', 'RECIPES',
           'SHAPES', 'RECORDS', 'OWN_SCALE', 'case_mask', 'default_scale', 'compare_np', 'ratios', 'check_planes', 'summary_np',
           'check_summary', 'known_states', 'check_known', 'draw_side', 'draw_pair', 'host_states']
