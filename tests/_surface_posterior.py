"""CPU restatement of the surface posterior, for the tests: contours and brute-force nearest squared
distances from tests/_hausdorff.py, the samples, the Welford recurrence in float64 and -- the same recurrence in the same order --
in float32, the maps and the per-label summary, and the tolerances.  No code shared with the HIP path.

The sample.  With a dyadic spacing every squared distance d2 is exact in float32, so the device's sample (float)sqrt((double)d2)
is the float32 rounding of the float64 sample s used here: |s32 - s| <= u |s|, u = 2^-24 (the double rounding through float64 adds
2^-53, far below).  Only the recurrence contributes beyond that.

The tolerances, for K samples at a voxel with |s| <= S (S = the largest |s| of the case).
  mean.  k = ++count; delta = s - mean; mean += delta / k in float32.  |mean| <= S, |delta| <= 2 S.  A step rounds three times:
  the difference by at most 2 u S, the quotient by 2 u S / k (and it carries the difference's error divided by k: 2 u S / k), the
  sum by u S: at most u S (1 + 4 / k).  An earlier error enters the next mean with the factor 1 - 1 / k <= 1, and the rounding of
  the samples moves their average by at most u S.  After K samples
      E_K = u S (K + 4 H_K + 1),  H_K = 1 + 1/2 + ... + 1/K.
  (Carrying the factor j / K an error of step j really has would halve this: the bound is not tight, and is kept as it is.)
  m2.  m2 += delta (s - mean_k).  Both factors are at most 2 S.  The computed delta differs from the float64 one by the error
  of the previous mean, its own rounding 2 u S and the sample's u S: E_{k-1} + 3 u S; the second factor likewise by E_k + 3 u S;
  the product rounds by 4 u S^2 and the sum by u m2_k <= u k S^2 (m2_k is a sum of k squared deviations from the mean, at most
  k S^2).  Step k adds at most 2 S (E_k + E_{k-1} + 6 u S) + 4 u S^2 + u k S^2 <= u S^2 (4 a_k + 16 + k), a_k = k + 4 H_k + 1:
      F_K = u S^2 sum_{k=1..K} (4 a_k + 16 + k).
  std = sqrtf(max(m2, 0) / (float)(K - 1)).  The clamp moves the float32 value towards the float64 one, which is >= 0.  With
  dv = F_K / (K - 1): |sqrt(a) - sqrt(b)| <= min(sqrt(|a - b|), |a - b| / sqrt(b)), so t = min(sqrt(dv), dv / std) bounds the
  propagated part, and the division and the root round by at most 2 u (std + t) together, held to 4 u (std + t).
The stated factor is 1: the tests hold the device, and the float32 evaluation here, to these bounds as they stand.
A sum column of the summary is held to the sum of its voxels' tolerances plus 1e-12 of its value (float64 sums in another order),
a maximum to the largest tolerance of its voxels; sum bias^2 to sum (2 |bias| + E) E."""
import functools
import statistics

import numpy as np

from tests import _hausdorff as HD

U = 2.0 ** -24
LABELS3 = [10, 16, 58]
INT_COLUMNS = 3
FLOAT_COLUMNS = 6


def z_of(levels):
    return [statistics.NormalDist().inv_cdf(0.5 * (1.0 + q)) for q in levels]


def samples(seg_fixed, seg_moving, labels, spacing):
    """seg_fixed (D,H,W), seg_moving (C,D,H,W) -> s (C,D,H,W) float64: the sample of chain c at every voxel of the fixed contour of
    a listed label, NaN where there is none (off the contours; the label absent from the chain's map)"""
    C = seg_moving.shape[0]
    s = np.full(seg_moving.shape, np.nan)
    for lab in labels:
        a = HD.contour(seg_fixed == lab)
        if not a.any():
            continue
        for c in range(C):
            b = HD.contour(seg_moving[c] == lab)
            if not b.any():
                continue
            d = np.sqrt(HD.nearest_d2(a, b, spacing))
            sign = np.where(seg_moving[c][a] == lab, -1.0, 1.0)
            s[c][a] = np.where(d == 0.0, 0.0, sign * d)
    return s


def welford(records, dtype, state=None):
    """records: iterable of (C,D,H,W) float64 sample arrays, one per step -> (mean, m2 of `dtype`, count int32): the recurrence
    of include/irsgmcmc.h at every voxel, chains in ascending order, a NaN sample skipped, every operation rounded to `dtype`"""
    records = list(records)
    shape = records[0].shape[1:]
    if state is None:
        mean, m2, count = np.zeros(shape, dtype), np.zeros(shape, dtype), np.zeros(shape, np.int32)
    else:
        mean, m2, count = (np.array(a) for a in state)
    for rec in records:
        for s in rec:
            has = ~np.isnan(s)
            x = s[has].astype(dtype)  # float32: the one rounding of the root
            count[has] += 1
            k = count[has].astype(dtype)
            delta = x - mean[has]
            mu = mean[has] + delta / k
            m2[has] = m2[has] + delta * (x - mu)
            mean[has] = mu
    return mean, m2, count


def maps(mean, m2, count):
    """-> (bias, std) of the dtype of the state: NaN where count == 0 / count < 2"""
    dtype = mean.dtype
    bias = np.where(count >= 1, mean, np.nan).astype(dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        std = np.sqrt((np.maximum(m2, dtype.type(0)) / np.maximum(count - 1, 1).astype(dtype)).astype(dtype)).astype(dtype)
    return bias, np.where(count >= 2, std, np.nan).astype(dtype)


def fixed_contours(seg_fixed, labels):
    """-> (D,H,W) int: the index in `labels` of the label whose fixed contour holds the voxel, -1 elsewhere"""
    li = np.full(seg_fixed.shape, -1)
    for j, lab in enumerate(labels):
        li[HD.contour(seg_fixed == lab)] = j
    return li


def summary(bias, std, count, seg_fixed, labels, levels, mask=None):
    """-> (isummary (L, 3 + len(levels)) int64, fsummary (L, 6) float64) of include/irsgmcmc.h, from float64 sums"""
    li = fixed_contours(seg_fixed, labels)
    if mask is not None:
        li = np.where(mask, li, -1)
    z = z_of(levels)
    isum = np.zeros((len(labels), INT_COLUMNS + len(levels)), np.int64)
    fsum = np.zeros((len(labels), FLOAT_COLUMNS))
    fsum[:, (3, 5)] = -np.inf
    for j in range(len(labels)):
        sel = li == j
        one, two = sel & (count >= 1), sel & (count >= 2)
        b, sd, b2 = bias[one].astype(np.float64), std[two].astype(np.float64), bias[two].astype(np.float64)
        isum[j, :3] = sel.sum(), one.sum(), two.sum()
        for q, zq in enumerate(z):
            isum[j, 3 + q] = (np.abs(b2) <= zq * sd).sum()
        fsum[j, :3] = b.sum(), np.abs(b).sum(), (b * b).sum()
        fsum[j, 4] = sd.sum()
        if len(b):
            fsum[j, 3] = np.abs(b).max()
        if len(sd):
            fsum[j, 5] = sd.max()
    return isum, fsum


# ------------------------------------------------------------------------------------------------ tolerances
def harmonic(K):
    K = np.asarray(K)
    return np.concatenate([[0.0], np.cumsum(1.0 / np.arange(1, (int(K.max()) if K.size else 0) + 1))])[K]


def _used(dev, tol):
    """the fraction of the bound a deviation uses, elementwise (a deviation where the bound is 0 counts as beyond it)"""
    return np.where(tol > 0, dev / np.where(tol > 0, tol, 1.0), np.where(dev > 0, np.inf, 0.0))


def mean_tol(K, S):
    """E_K of the module docstring; K: int array of sample counts"""
    K = np.asarray(K)
    return U * S * (K + 4.0 * harmonic(K) + 1.0) * (K > 0)


def m2_tol(K, S):
    """F_K of the module docstring"""
    K = np.asarray(K)
    k = np.arange(1, (int(K.max()) if K.size else 0) + 1)
    a = k + 4.0 * harmonic(k) + 1.0
    steps = np.concatenate([[0.0], np.cumsum(4.0 * a + 16.0 + k)])
    return U * S * S * steps[K]


def std_tol(K, S, std_ref):
    """the bound of std for count K >= 2 around the float64 value std_ref (arrays of one shape)"""
    K = np.asarray(K)
    dv = m2_tol(K, S) / np.maximum(K - 1, 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.minimum(np.sqrt(dv), np.where(std_ref > 0, dv / std_ref, np.inf))
    return t + 4.0 * U * (std_ref + t)


def summary_tol(bias, std, count, seg_fixed, labels, S, mask=None):
    """-> (L, 6) float64: the tolerance of every float column of summary() around its float64 value"""
    li = fixed_contours(seg_fixed, labels)
    if mask is not None:
        li = np.where(mask, li, -1)
    tol = np.zeros((len(labels), FLOAT_COLUMNS))
    for j in range(len(labels)):
        sel = li == j
        one, two = sel & (count >= 1), sel & (count >= 2)
        e = mean_tol(count[one], S)
        b = np.abs(bias[one].astype(np.float64))
        t = std_tol(count[two], S, std[two].astype(np.float64))
        tol[j] = [e.sum() + 1e-12 * b.sum(), e.sum() + 1e-12 * b.sum(), ((2.0 * b + e) * e).sum() + 1e-12 * (b * b).sum(),
                  e.max() if e.size else 0.0, t.sum() + 1e-12 * std[two].astype(np.float64).sum(), t.max() if t.size else 0.0]
    return tol


# ------------------------------------------------------------------------------------------------ the cases
# (1,1,3): one row; (5,7,9): ragged; (9,11,70): a box wider than one 64-lane chunk; (70,9,5) and (3,70,6): lines longer than the
# LDS envelope (64), along z and along y, so the envelopes live in global scratch
SHAPES = [(1, 1, 3), (5, 7, 9), (9, 11, 70), (70, 9, 5), (3, 70, 6)]
CHAINS = [1, 2, 3]
STEPS = 3
SPACINGS = [(1.0, 1.0, 1.0), (0.5, 1.0, 2.0)]  # dyadic: every squared distance is exact in float32


def _seg(rng, dims, labels):
    if np.prod(dims) < 27:  # a row of voxels: blobs would fill it
        return rng.choice(np.array([0] + list(labels[:2]), np.int16), size=dims)
    if min(dims) >= 4:
        return HD.random_seg(rng, dims, labels)  # structures touch the volume border
    # HD.random_seg draws its radii from [1, min(dims) / 4]: a volume thinner than 4 gets the same blobs with per-axis radii
    seg = np.zeros(dims, np.int16)
    z, y, x = np.meshgrid(*(np.arange(n) for n in dims), indexing='ij')
    for lab in labels:
        for _ in range(rng.integers(1, 3)):
            c = rng.uniform(0, 1, 3) * np.array(dims)
            r = rng.uniform(1.0, np.maximum(2.0, 0.25 * np.array(dims)))
            blob = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 < 1.0
            seg[blob & (rng.uniform(size=dims) < 0.995)] = lab
    seg[:, 0, :3] = labels[0]
    return seg


@functools.lru_cache(maxsize=None)
def case_maps(dims, C):
    """-> (fixed (D,H,W) int16, moving (STEPS, C, D, H, W) int16, mask (D,H,W) bool), the same for every test that asks"""
    rng = np.random.default_rng([11, C, *dims])
    while True:
        fixed = _seg(rng, dims, LABELS3)
        if fixed_contours(fixed, LABELS3).max() >= 0:
            break
    moving = np.stack([np.stack([_seg(rng, dims, LABELS3) for _ in range(C)]) for _ in range(STEPS)])
    mask = rng.uniform(size=dims) < 0.7
    for a in (fixed, moving, mask):
        a.setflags(write=False)
    return fixed, moving, mask


@functools.lru_cache(maxsize=None)
def case_reference(dims, C, spacing):
    """the float64 restatement of case_maps(dims, C) at `spacing`, computed once and left unchanged: dict with 's' (the samples
    of every step), 'S' (the largest |s|), 'mean', 'm2', 'count', 'bias', 'std'"""
    fixed, moving, _ = case_maps(dims, C)
    s = [samples(fixed, moving[t], LABELS3, spacing) for t in range(STEPS)]
    mean, m2, count = welford(s, np.float64)
    bias, std = maps(mean, m2, count)
    ref = {'s': np.stack(s), 'mean': mean, 'm2': m2, 'count': count, 'bias': bias, 'std': std}
    for v in ref.values():
        v.setflags(write=False)
    ref['S'] = float(np.nanmax(np.abs(ref['s']))) if np.isfinite(ref['s']).any() else 0.0
    return ref


def check_state(test, check, got_mean, got_m2, got_count, ref, S):
    """every contour voxel against the float64 restatement within the bounds, the counts for equality everywhere; `check`:
    tests._report.check or a stand-in with its signature.  -> the largest fraction of a bound used"""
    assert np.array_equal(got_count, ref['count'])
    on = ref['count'] > 0
    if not on.any():
        return 0.0
    dm = np.abs(got_mean[on].astype(np.float64) - ref['mean'][on])
    d2 = np.abs(got_m2[on].astype(np.float64) - ref['m2'][on])
    um, u2 = _used(dm, mean_tol(ref['count'][on], S)), _used(d2, m2_tol(ref['count'][on], S))
    check(test, 'mean / bound', um, 0.0, 1.0)
    check(test, 'm2 / bound', u2, 0.0, 1.0)
    return float(max(um.max(), u2.max()))


def check_maps(test, check, got_bias, got_std, ref, S):
    assert np.array_equal(np.isnan(got_bias), np.isnan(ref['bias'])) and np.array_equal(np.isnan(got_std), np.isnan(ref['std']))
    one, two = ref['count'] >= 1, ref['count'] >= 2
    if one.any():
        db = np.abs(got_bias[one].astype(np.float64) - ref['bias'][one])
        check(test, 'bias / bound', _used(db, mean_tol(ref['count'][one], S)), 0.0, 1.0)
    if two.any():
        ds = np.abs(got_std[two].astype(np.float64) - ref['std'][two])
        check(test, 'std / bound', _used(ds, std_tol(ref['count'][two], S, ref['std'][two])), 0.0, 1.0)


def check_summary(test, check, got_i, got_f, got_bias, got_std, ref, fixed, labels, levels, S, mask=None):
    """the integer columns for equality (the coverage columns against the call's OWN maps, compared in float64 as the device does,
    and inside the band the tolerances of the restatement's maps leave), the float columns within summary_tol"""
    want_i, want_f = summary(ref['bias'], ref['std'], ref['count'], fixed, labels, levels, mask)
    assert np.array_equal(got_i[:, :3], want_i[:, :3])
    own_i, _ = summary(got_bias, got_std, ref['count'], fixed, labels, levels, mask)
    assert np.array_equal(got_i[:, 3:3 + len(levels)], own_i[:, 3:]) and not got_i[:, 3 + len(levels):].any()
    li = fixed_contours(fixed, labels)
    if mask is not None:
        li = np.where(mask, li, -1)
    for j in range(len(labels)):
        two = (li == j) & (ref['count'] >= 2)
        b, sd = np.abs(ref['bias'][two]), ref['std'][two]
        e, t = mean_tol(ref['count'][two], S), std_tol(ref['count'][two], S, sd)
        for q, zq in enumerate(z_of(levels)):
            lo, hi = (b + e <= zq * (sd - t)).sum(), (b - e <= zq * (sd + t)).sum()
            assert lo <= got_i[j, 3 + q] <= hi, (test, j, q, lo, int(got_i[j, 3 + q]), hi)
    tol = summary_tol(ref['bias'], ref['std'], ref['count'], fixed, labels, S, mask)
    empty = np.isinf(want_f)
    assert np.array_equal(np.isinf(got_f), empty) and np.array_equal(got_f[empty], want_f[empty])
    dev = np.where(empty, 0.0, np.abs(np.where(empty, 0.0, got_f) - np.where(empty, 0.0, want_f)))
    check(test, 'summary / bound', _used(dev, tol), 0.0, 1.0)


# ------------------------------------------------------------------------------------------------ known answers
def half_spaces(dims, a, b, lab=16):
    """fixed labels x < a, moving x < b (x: the last axis) -> (fixed (D,H,W), moving (1,D,H,W)); s = (a - b) sx on the contour"""
    f, m = np.zeros(dims, np.int16), np.zeros((1,) + tuple(dims), np.int16)
    f[:, :, :a] = lab
    m[:, :, :, :b] = lab
    return f, m


def single_voxels(dims, p, q, lab=10):
    """one voxel of the label at p in the fixed map and at q in the moving one; s = +|(p - q) * spacing| at p"""
    f, m = np.zeros(dims, np.int16), np.zeros((1,) + tuple(dims), np.int16)
    f[p] = lab
    m[(0,) + tuple(q)] = lab
    return f, m


def point_distance(p, q, spacing):
    """|(p - q) * spacing| with p, q as (z, y, x) and spacing as (sx, sy, sz)"""
    return float(np.sqrt(sum(((pi - qi) * s) ** 2 for pi, qi, s in zip(p, q, spacing[::-1]))))


# ------------------------------------------------------------------------------------------------ refusals of the C ABI
def abi_refusals():
    """(entry point, replaced arguments, expected irs_last_error()) of every refusal that happens before any HIP call: device
    pointers are a dummy non-null address the checks never dereference, the host arrays they read are real"""
    import ctypes as C
    from ir_sgmcmc_amd import _lib as L
    P = 0x1000
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    f3 = lambda *v: (C.c_float * 3)(*v)
    f64 = lambda *v: (C.c_double * len(v))(*v)
    U, F, W = 'irs_surface_posterior_update', 'irs_surface_posterior_finalize', 'irs_surface_posterior_workspace'
    nan, inf = float('nan'), float('inf')
    cases = []
    for arg in ('seg_fixed', 'seg_moving', 'spacing', 'workspace', 'mean', 'm2', 'count'):
        cases.append((U, {arg: None}, f'{U}: bad arguments'))
    for arg in ('seg_fixed', 'mean', 'm2', 'count', 'bias', 'std', 'isummary', 'fsummary', 'ws'):
        cases.append((F, {arg: None}, f'{F}: bad arguments'))
    for fn in (U, F):
        cases.append((fn, {'D': 0}, f'{fn}: bad arguments'))
        cases.append((fn, {'D': 1 << 10, 'H': 1 << 10, 'W': 1 << 10}, f'{fn}: bad arguments'))
        msg = f'{fn}: 1..{L.IRS_MAX_LABELS} labels in the int16 range'
        cases += [(fn, {'labels': None}, msg), (fn, {'n_labels': 0}, msg), (fn, {'labels': i32(1, 40000)}, msg),
                  (fn, {'labels': i32(*range(L.IRS_MAX_LABELS + 1)), 'n_labels': L.IRS_MAX_LABELS + 1}, msg),
                  (fn, {'labels': i32(7, 7)}, f'{fn}: label 7 appears twice')]
    for C_ in (0, L.IRS_MAX_CHAINS + 1):
        cases.append((U, {'C': C_}, f'{U}: C = {C_} chains, 1..{L.IRS_MAX_CHAINS}'))
    for a in range(3):
        for v, shown in ((0.0, '0'), (-1.0, '-1'), (nan, 'nan'), (inf, 'inf')):
            sp = [1.0, 1.0, 1.0]
            sp[a] = v
            cases.append((U, {'spacing': f3(*sp)}, f'{U}: spacing[{a}] = {shown}, a finite value > 0 needed'))
    cases += [(U, {'boxes': None}, 'irs_surface_distance: bad boxes / dims'),
              (U, {'boxes': i32(*([0, 0, 0, 3, 3, 4] * 4))}, 'irs_surface_distance: box 0 out of the volume'),
              (U, {'workspace_bytes': 0}, None),  # the message names the bytes needed: matched by its head and tail
              (W, {'bytes': None}, f'{W}: null argument'), (W, {'boxes': None}, 'irs_surface_distance: bad boxes / dims'),
              (W, {'n_pairs': 0}, 'irs_surface_distance: bad boxes / dims'), (W, {'W': 0}, 'irs_surface_distance: bad boxes / dims')]
    for n in (-1, L.IRS_SURFACE_MAX_LEVELS + 1):
        cases.append((F, {'n_levels': n, 'z': f64(*([1.0] * 5))}, f'{F}: 0..4 coverage levels with their z, got {n}'))
    cases.append((F, {'z': None}, f'{F}: 0..4 coverage levels with their z, got 2'))
    for v, shown in ((0.0, '0'), (-1.0, '-1'), (nan, 'nan'), (inf, 'inf')):
        cases.append((F, {'z': f64(1.0, v)}, f'{F}: z[1] = {shown}, a finite value > 0 needed'))
    cases.append((F, {'ws_bytes': L.IRS_SURFACE_WS_BYTES - 1},
                  f'{F}: workspace of {L.IRS_SURFACE_WS_BYTES - 1} bytes, {L.IRS_SURFACE_WS_BYTES} needed (IRS_SURFACE_WS_BYTES)'))
    return cases


def assert_refused(fn, bad, message):
    import ctypes as C
    from ir_sgmcmc_amd import _lib as L
    P = 0x1000
    i32 = lambda *v: (C.c_int32 * len(v))(*v)
    size = C.c_size_t()
    dims = dict(D=4, H=4, W=4)
    boxes = i32(*([0, 0, 0, 3, 3, 3] * 4))  # C = 2 chains x 2 labels, each box the whole 4^3 volume
    good = {
        'irs_surface_posterior_workspace': dict(boxes=boxes, n_pairs=4, **dims, bytes=C.byref(size)),
        'irs_surface_posterior_update': dict(seg_fixed=P, seg_moving=P, labels=i32(1, 2), n_labels=2, spacing=(C.c_float * 3)(1, 1, 1),
                                             boxes=boxes, workspace=P, workspace_bytes=1 << 30, mean=P, m2=P, count=P, C=2, **dims,
                                             stream=None),
        'irs_surface_posterior_finalize': dict(seg_fixed=P, labels=i32(1, 2), n_labels=2, mean=P, m2=P, count=P, mask=None,
                                               z=(C.c_double * 2)(0.67, 1.96), n_levels=2, bias=P, std=P, isummary=P, fsummary=P, ws=P,
                                               ws_bytes=L.IRS_SURFACE_WS_BYTES, **dims, stream=None),
    }[fn]
    assert set(bad) <= set(good), (fn, bad)
    lib = L.load()
    assert getattr(lib, fn)(*{**good, **bad}.values()) != 0
    err = lib.irs_last_error().decode()
    if message is None:
        assert err.startswith(f'{fn}: workspace of 0 bytes, ') and err.endswith(' needed (irs_surface_posterior_workspace)'), err
    else:
        assert err == message, err
