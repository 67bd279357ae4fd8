"""numpy restatement of the displacement covariance posterior ("Displacement covariance"), the input
recipes, the tolerances and the checks, shared by the host and GPU tests.

The reference runs the Welford recurrences of the definitions in float64 (the inputs are float32 and exact), forms
S_ab = scale_a scale_b M_ab / max(n - 1, 1) and hands it to numpy.linalg.eigh.

Forward bound E on |S32 - S|_F for a float32 evaluation of the state in the kernel's operation order; u = 2^-24.
  mean.  mu_k = fl(mu_{k-1} + fl(fl(x - mu_{k-1}) / k)): the difference and the quotient round a value of size <= R / k after
    the division (R the range of the channel's records), the sum a value of size <= X = max |x|, and the recurrence itself
    damps the earlier error by (1 - 1/k):  err_k <= (1 - 1/k) err_{k-1} + u (2 R / k + X),  err_1 = 0
        =>  err_k <= Em := u (2 R + X (n + 1) / 2)   for every k <= n.
  co-moment.  M_ab = sum_k delta_a e_b with delta_a = x_a - mu_a (old mean), e_b = x_b - mu_b (new mean).  The computed delta_a
    is off by at most Em_a, e_b by Em_b (the propagated error of the mean), and each term carries one rounding of delta, one of
    e, one of the product and at most n - 1 of the running sum: n + 2 roundings, gamma_m = m u / (1 - m u):
        dM_ab = gamma_{n+2} A_ab + Em_b sum_k |delta_a| + Em_a sum_k |e_b| + n Em_a Em_b,   A_ab = sum_k |delta_a e_b|,
    all sums running sums of the float64 reference.  A fused multiply-add drops a rounding and never adds one.
  dS_ab = scale_a scale_b dM_ab / max(n - 1, 1), and E = FACTOR * sqrt(sum_a dS_aa^2 + 2 sum_{a<b} dS_ab^2), FACTOR = 2 for the
  second-order terms left out above and for the double-precision solver (whose error, 2e-16 |S|_F, is far below u).

What the maps are held to, by perturbation theory (lambda_1 >= lambda_2 >= lambda_3 the reference eigenvalues, |lambda|_2
their 2-norm; the *stored* float32 std, direction and anisotropy of the device enter, widened to float64):
  eigenvalues   |std_i^2 - lambda_i| <= E + 2^-22 lambda_i.  Weyl: the i-th eigenvalue moves by at most |dS|_2 <= E; clamping
                at 0 moves it towards lambda_i >= 0; the float32 square root and its squaring back cost (1 + u)^2 - 1 < 2^-22.
  direction     unit norm within 4 * 2^-24 (three components rounded to float32), or exactly zero where lambda_1 = 0.
  residual      |S d - std_0^2 d|_2 <= 2 E + 2^-21 |S|_F with S the reference matrix, d the stored direction and std_0 the
                stored major std.  With (l, v) the exact major pair of the device's matrix S':  S d - std_0^2 d =
                (S - S') d + (S' - l)(d - v) + (l - std_0^2) d, and |S - S'| <= E, |d - v| <= sqrt(3) u, |l - std_0^2| <=
                2^-22 l.  Well-conditioned even where lambda_1 ~ lambda_2.
  eigenvector   only where (lambda_1 - lambda_2) / lambda_1 >= GAP = 0.05:  sin angle(d, v_ref) <= 2 E / (lambda_1 - lambda_2)
                (Davis-Kahan in the form of Yu, Wang and Samworth 2015) + 2^-22 for the float32 storage.
  anisotropy    FA = sqrt(3/2) g(lambda), g = |P lambda|_2 / |lambda|_2 with P the projector off the constant vector.  For
                lambda' = lambda + D:  |g(lambda') - g(lambda)| <= |D|_2 / |lambda|_2 + g |D|_2 / |lambda|_2 <= 2 |D|_2 /
                |lambda|_2, and Weyl bounds each of the three entries of D by E, so |D|_2 <= sqrt(3) E and
                    |dFA| <= sqrt(3/2) * 2 * sqrt(3) * E / |lambda|_2 = 3 sqrt(2) E / |lambda|_2,
                the constant of the definitions.  (Hoffman-Wielandt would give sqrt(6).)  The float32 storage of FA, u FA, is
                inside it: A_aa scale_a^2 / (n - 1) = S_aa, so E >= 2 gamma_4 sqrt(sum S_aa^2) >= 8 u |lambda|_2 / sqrt(3).
                Compared only where the bound is <= FA_BOUND = 0.05.
"""
import numpy as np

U = 2.0 ** -24
FACTOR = 2.0
GAP = 0.05
FA_BOUND = 0.05
SWEEPS = 5
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # the order of the six co-moments


def default_scale(shape):
    """normalised coordinates -> voxels for channels x, y, z of a (D, H, W) volume"""
    D, H, W = shape
    return ((W - 1) / 2, (H - 1) / 2, (D - 1) / 2)


def welford_np(records, dtype=np.float64):
    """the update's recurrences in `dtype` numpy (no fused multiply-add): records (n,3,...) float32 in order ->
    mean (3,...), M (6,...) and, as float64 running sums of the absolute terms, A (6,...), sum |delta| (3,...), sum |e| (3,...)"""
    records = np.asarray(records, dtype=np.float32)
    n = records.shape[0]
    shape = records.shape[2:]
    mean = np.zeros((3,) + shape, dtype=dtype)
    M = np.zeros((6,) + shape, dtype=dtype)
    A = np.zeros((6,) + shape)
    sd = np.zeros((3,) + shape)
    se = np.zeros((3,) + shape)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(1, n + 1):
            x = records[k - 1].astype(dtype)
            if k == 1:
                mean = x.copy()
                M[:] = 0
                continue
            d = (x - mean).astype(dtype)
            mean = (mean + (d / dtype(k)).astype(dtype)).astype(dtype)
            e = (x - mean).astype(dtype)
            for j, (a, b) in enumerate(PAIRS):
                t = (d[a] * e[b]).astype(dtype)
                M[j] = (M[j] + t).astype(dtype)
                A[j] += np.abs(t.astype(np.float64))
            sd += np.abs(d.astype(np.float64))
            se += np.abs(e.astype(np.float64))
    return mean, M, A, sd, se


def matrices(M, n, scale):
    """M (6,...) -> S (...,3,3) float64: scale_a scale_b M_ab / max(n - 1, 1)"""
    M = np.asarray(M, dtype=np.float64)
    S = np.empty(M.shape[1:] + (3, 3))
    for j, (a, b) in enumerate(PAIRS):
        S[..., a, b] = S[..., b, a] = scale[a] * scale[b] * M[j] / max(n - 1, 1)
    return S


def sign_rule(v):
    """v (...,3): the component of largest magnitude made positive, the lowest channel on a tie"""
    i = np.argmax(np.abs(v), axis=-1)  # the first maximum
    big = np.take_along_axis(v, i[..., None], axis=-1)
    return np.where(big < 0, -v, v)


def fractional_anisotropy(lam):
    """lam (...,3) >= 0 -> sqrt(3/2 sum (l - mean)^2 / sum l^2), 0 where the denominator is 0"""
    den = (lam ** 2).sum(axis=-1)
    num = ((lam - lam.mean(axis=-1, keepdims=True)) ** 2).sum(axis=-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den > 0, np.sqrt(1.5 * num / np.where(den > 0, den, 1.0)), 0.0)


def maps_from_eigen(lam, vec, finite):
    """lam (...,3) descending, vec (...,3) the major eigenvector -> std (3,...), direction (3,...), anisotropy (...) float64;
    NaN where ~finite"""
    lam = np.maximum(lam, 0.0)
    std = np.sqrt(lam)
    d = np.where((lam[..., :1] > 0), sign_rule(vec), 0.0)
    fa = fractional_anisotropy(lam)
    nan = np.nan
    return (np.where(finite, np.moveaxis(std, -1, 0), nan), np.where(finite, np.moveaxis(d, -1, 0), nan), np.where(finite, fa, nan))


def eigh_desc(S):
    """numpy.linalg.eigh, eigenvalues descending: -> lam (...,3), vectors (...,3,3) with column i the i-th eigenvector"""
    lam, vec = np.linalg.eigh(S)
    return lam[..., ::-1], vec[..., ::-1]


def jacobi_np(S, sweeps=SWEEPS):
    """the finalize's cyclic Jacobi iteration, float64: pairs (0,1), (0,2), (1,2) per sweep, a fixed number of sweeps, the
    identity rotation where the off-diagonal entry is exactly 0.  S (...,3,3) -> (lam (...,3) descending and not clamped,
    vectors (...,3,3) with column i the i-th eigenvector, off-diagonal norm left)"""
    A = np.array(S, dtype=np.float64)
    V = np.zeros_like(A)
    V[..., 0, 0] = V[..., 1, 1] = V[..., 2, 2] = 1.0
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = A[..., p, q].copy()
                tau = (A[..., q, q] - A[..., p, p]) / (2.0 * apq)
                t = 1.0 / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                t = np.where(tau < 0, -t, t)
                t = np.where(apq == 0, 0.0, t)
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                A[..., p, p] -= t * apq
                A[..., q, q] += t * apq
                A[..., p, q] = A[..., q, p] = 0.0
                arp, arq = A[..., r, p].copy(), A[..., r, q].copy()
                A[..., r, p] = A[..., p, r] = c * arp - s * arq
                A[..., r, q] = A[..., q, r] = s * arp + c * arq
                vp, vq = V[..., :, p].copy(), V[..., :, q].copy()
                V[..., :, p] = c[..., None] * vp - s[..., None] * vq
                V[..., :, q] = s[..., None] * vp + c[..., None] * vq
    lam = np.stack([A[..., 0, 0], A[..., 1, 1], A[..., 2, 2]], axis=-1)
    off = np.sqrt(2 * (A[..., 0, 1] ** 2 + A[..., 0, 2] ** 2 + A[..., 1, 2] ** 2))
    order = np.argsort(-lam, axis=-1, kind='stable')
    lam = np.take_along_axis(lam, order, axis=-1)
    V = np.take_along_axis(V, order[..., None, :], axis=-1)
    return lam, V, off


def finalize_np(mean, M, n, scale, solver='jacobi'):
    """the finalize from a given state (whatever precision it was accumulated in), in float64 -> std, direction (3,...),
    anisotropy (...) rounded to float32 as the device stores them"""
    mean, M = np.asarray(mean), np.asarray(M)
    finite = np.isfinite(mean).all(axis=0) & np.isfinite(M).all(axis=0)
    S = matrices(np.where(finite, M, 0.0), n, scale)
    lam, vec = (jacobi_np(S)[:2] if solver == 'jacobi' else eigh_desc(S))
    std, d, fa = maps_from_eigen(lam, vec[..., :, 0], finite)
    d32 = d.astype(np.float32)
    # the sign rule is applied to the stored values
    d32 = np.moveaxis(np.where(finite[..., None], sign_rule(np.moveaxis(d32, 0, -1)), np.nan), -1, 0).astype(np.float32)
    return std.astype(np.float32), d32, fa.astype(np.float32)


def summary_np(n, std, direction, anisotropy, mask=None):
    """the summary over `mask` of the given maps (float64 sums of whatever values they hold)"""
    std, direction, anisotropy = (np.asarray(x, dtype=np.float64) for x in (std, direction, anisotropy))
    m = np.ones(anisotropy.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    voxels = int(m.sum())
    fin = m & np.isfinite(anisotropy)
    k = int(fin.sum())
    nan = float('nan')
    if k == 0:
        vals = dict.fromkeys(('std_major_mean', 'std_major_max', 'std_total_mean', 'anisotropy_mean', 'anisotropy_max', 'dir_x',
                              'dir_y', 'dir_z'), nan)
    else:
        s = std[:, fin]
        vals = {'std_major_mean': float(s[0].sum() / k), 'std_major_max': float(s[0].max()),
                'std_total_mean': float(np.sqrt((s ** 2).sum(axis=0)).sum() / k),
                'anisotropy_mean': float(anisotropy[fin].sum() / k), 'anisotropy_max': float(anisotropy[fin].max()),
                **{f'dir_{c}': float(np.abs(direction[i][fin]).sum() / k) for i, c in enumerate('xyz')}}
    return {'records': int(n), 'voxels': voxels, 'nonfinite_voxels': voxels - k, **vals}


def covariance_np(records, scale=None, mask=None):
    """records (n,3,D,H,W) float32 in record order (steps, chains within a step) -> dict of the float64 reference: mean, M,
    S (D,H,W,3,3), lam (D,H,W,3) descending, vec (D,H,W,3) the major eigenvector, E (D,H,W) the forward bound of the module
    docstring, dM (6,D,H,W) its per-entry bound on the co-moments (without FACTOR), std, direction, anisotropy and the summary of those maps"""
    records = np.asarray(records, dtype=np.float32)
    n, shape = records.shape[0], records.shape[2:]
    scale = default_scale(shape) if scale is None else tuple(float(s) for s in scale)
    mean, M, A, sd, se = welford_np(records)
    finite = np.isfinite(records).all(axis=(0, 1))
    S = matrices(np.where(finite, M, 0.0), n, scale)
    lam, vecs = eigh_desc(S)
    lam = np.maximum(lam, 0.0)
    vec = vecs[..., :, 0]
    std, direction, fa = maps_from_eigen(lam, vec, finite)
    # the bound
    x = np.where(finite, records.astype(np.float64), 0.0)
    R = x.max(axis=0) - x.min(axis=0)
    X = np.abs(x).max(axis=0)
    Em = U * (2 * R + X * (n + 1) / 2)
    m = n + 2
    gamma = m * U / (1 - m * U)
    sq = np.zeros(shape)
    dMs = np.zeros((6,) + tuple(shape))
    with np.errstate(invalid='ignore', over='ignore'):  # non-finite voxels are masked out below
        for j, (a, b) in enumerate(PAIRS):
            dM = gamma * A[j] + Em[b] * sd[a] + Em[a] * se[b] + n * Em[a] * Em[b]
            dMs[j] = dM
            dS = scale[a] * scale[b] * dM / max(n - 1, 1)
            sq += (1 if a == b else 2) * dS ** 2
    E = FACTOR * np.sqrt(np.where(finite, sq, 0.0))
    return {'n': n, 'scale': scale, 'finite': finite, 'mean': mean, 'M': M, 'S': S, 'lam': lam, 'vec': vec, 'E': E, 'dM': dMs, 'std': std,
            'direction': direction, 'anisotropy': fa, 'summary': summary_np(n, std, direction, fa, mask)}


def check_maps(ref, std, direction, anisotropy, compare_eigenvector=True, max_gap_share=0.005, all_fa=True):
    """hold the stored float32 maps (std (3,...), direction (3,...), anisotropy (...)) to the tolerances of the module
    docstring; prints, then asserts.  -> the figures: name -> (worst error, worst error / tolerance)"""
    fin = ref['finite']
    std, direction, anisotropy = (np.asarray(x) for x in (std, direction, anisotropy))
    assert std.dtype == np.float32 and direction.dtype == np.float32 and anisotropy.dtype == np.float32
    for plane in (*std, *direction, anisotropy):
        assert np.isnan(plane[~fin]).all() and np.isfinite(plane[fin]).all()
    lam, E, S = ref['lam'][fin], ref['E'][fin], ref['S'][fin]
    s = std.astype(np.float64)[:, fin].T            # (v, 3)
    d = direction.astype(np.float64)[:, fin].T      # (v, 3)
    fa = anisotropy.astype(np.float64)[fin]
    figures = {'voxels': int(fin.sum())}
    tiny = 1e-300

    def figure(name, err, tol):
        figures[name] = (float(err.max()), float((err / np.maximum(tol, tiny)).max())) if err.size else (0.0, 0.0)

    figure('eigenvalues', np.abs(s ** 2 - lam), E[:, None] + 2.0 ** -22 * lam)
    assert (np.diff(s, axis=1) <= 0).all()  # descending
    zero = lam[:, 0] == 0
    assert (d[zero] == 0).all()
    norm = np.sqrt((d ** 2).sum(axis=1))
    figure('direction norm', np.abs(norm - 1)[~zero], np.full((~zero).sum(), 4 * U))
    normS = np.sqrt((S ** 2).sum(axis=(1, 2)))
    res = np.einsum('vab,vb->va', S, d) - (s[:, :1] ** 2) * d
    figure('direction residual', np.sqrt((res ** 2).sum(axis=1)), 2 * E + 2.0 ** -21 * normS)
    gap = lam[:, 0] - lam[:, 1]
    with np.errstate(invalid='ignore', divide='ignore'):
        wide = ~zero & (gap >= GAP * lam[:, 0])
    figures['share with gap < 0.05'] = float((~zero & ~wide).mean()) if fin.any() else 0.0
    if compare_eigenvector:
        v = ref['vec'][fin]
        sin = np.sqrt((np.cross(d, v) ** 2).sum(axis=1))[wide]
        tol = 2 * E[wide] / gap[wide] + 2.0 ** -22
        figure('eigenvector sine', sin, tol)
        # the sign: where the reference's largest component leads the next by more than the eigenvector may move
        a = np.sort(np.abs(v[wide]), axis=1)
        clear = a[:, 2] - a[:, 1] > 4 * tol
        assert ((d[wide] * sign_rule(v[wide])).sum(axis=1)[clear] > 0).all()
    norml = np.sqrt((lam ** 2).sum(axis=1))
    with np.errstate(invalid='ignore', divide='ignore'):
        tol_fa = np.where(norml > 0, 3 * np.sqrt(2.0) * E / np.where(norml > 0, norml, 1.0), 0.0)
    held = tol_fa <= FA_BOUND
    figures['share left out of FA'] = float((~held).mean()) if fin.any() else 0.0
    figure('anisotropy', np.abs(fa - ref['anisotropy'][fin])[held], tol_fa[held])
    print(figures)  # worst error and worst error / tolerance, before the assertions
    for name in ('eigenvalues', 'direction norm', 'direction residual', 'anisotropy') + (('eigenvector sine',) if compare_eigenvector else ()):
        assert figures[name][1] <= 1.0, (name, figures[name])
    if compare_eigenvector:
        assert figures['share with gap < 0.05'] <= max_gap_share, figures  # a condition on the inputs
    if all_fa:
        assert figures['share left out of FA'] == 0.0, figures  # a condition on the inputs
    return figures


# ---------------------------------------------------------------- input recipes
def _upsample(coarse, shape):
    """trilinear, corners aligned: coarse (c, g, g, g) -> (c, D, H, W)"""
    out = coarse
    for axis, N in zip((1, 2, 3), shape):
        g = out.shape[axis]
        pos = np.linspace(0, g - 1, N)
        i0 = np.minimum(pos.astype(int), g - 2)
        w = (pos - i0).reshape([-1 if a == axis else 1 for a in range(4)])
        out = np.take(out, i0, axis=axis) * (1 - w) + np.take(out, i0 + 1, axis=axis) * w
    return out


def _to_normalised(d, shape):
    D, H, W = shape
    return d * np.array([2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1)]).reshape(3, 1, 1, 1)


def _rotations(rng, shape):
    """(D,H,W,3,3): a rotation per voxel, Rz(a) Ry(b) Rx(c) with smooth angle fields"""
    ang = _upsample(rng.uniform(-np.pi, np.pi, size=(3, 3, 3, 3)), shape)
    ca, sa, cb, sb, cc, sc = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    Rm = np.empty(tuple(shape) + (3, 3))
    Rm[..., 0, 0], Rm[..., 0, 1], Rm[..., 0, 2] = ca * cb, ca * sb * sc - sa * cc, ca * sb * cc + sa * sc
    Rm[..., 1, 0], Rm[..., 1, 1], Rm[..., 1, 2] = sa * cb, sa * sb * sc + ca * cc, sa * sb * cc - ca * sc
    Rm[..., 2, 0], Rm[..., 2, 1], Rm[..., 2, 2] = -sb, cb * sc, cb * cc
    return Rm


MEAN_AMPLITUDE = 2.0   # voxels: the smooth mean field's largest component
NOISE_AMPLITUDE = 0.25  # voxels: the unit of the per-record noise


def draw_records(recipe, n, shape, seed):
    """n records (n, 3, D, H, W) float32, normalised coordinates.  'anisotropic': a smooth mean field of MEAN_AMPLITUDE voxels
    plus, per record, noise N(0, diag(3, 2, 1)^2) * NOISE_AMPLITUDE voxels rotated by a rotation that varies per voxel.
    'white': the same mean plus isotropic N(0, 1) * NOISE_AMPLITUDE voxels."""
    rng = np.random.default_rng(seed)
    mean = _upsample(rng.uniform(-1, 1, size=(3, 4, 4, 4)), shape)
    mean *= MEAN_AMPLITUDE / np.abs(mean).max()
    Rm = _rotations(rng, shape)
    out = []
    for _ in range(n):
        z = rng.standard_normal(size=tuple(shape) + (3,))
        if recipe == 'anisotropic':
            noise = np.einsum('...ab,...b->...a', Rm, z * np.array([3.0, 2.0, 1.0]))
        elif recipe == 'white':
            noise = z
        else:
            raise ValueError(recipe)
        out.append(_to_normalised(mean + NOISE_AMPLITUDE * np.moveaxis(noise, -1, 0), shape).astype(np.float32))
    return np.stack(out)


def hand_checked_records(shape=(3, 4, 5), a=2.0, b=1.0, rotate=False):
    """(a,0,0), (-a,0,0), (0,b,0), (0,-b,0) at every voxel; `rotate`: by 45 degrees in the xy plane"""
    r = np.sqrt(0.5)
    pts = [(a, 0, 0), (-a, 0, 0), (0, b, 0), (0, -b, 0)]
    if rotate:
        pts = [(r * x - r * y, r * x + r * y, z) for x, y, z in pts]
    return np.stack([np.broadcast_to(np.array(p, dtype=np.float32).reshape(3, 1, 1, 1), (3,) + tuple(shape)) for p in pts]).copy()


HAND_STD = (np.sqrt(8 / 3), np.sqrt(2 / 3), 0.0)
HAND_FA = float(np.sqrt(1.5 * 312 / 612))  # lambda = (8/3, 2/3, 0): 0.874475

# C, steps, shape: every chain count, 1 to 5 steps, 2 x 2 x 3 to 64^3, volumes whose voxel count is and is not a multiple of 4
CASES = [
    (1, 1, (2, 2, 3)),
    (2, 3, (3, 4, 5)),
    (3, 2, (5, 7, 9)),
    (8, 1, (5, 7, 9)),
    (2, 5, (17, 16, 33)),
    (1, 4, (9, 7, 70)),
    (3, 3, (32, 32, 32)),
    (8, 5, (24, 40, 65)),
    (2, 2, (64, 64, 64)),
]
RECIPES = ('anisotropic', 'white')


def case_seed(C, steps, shape, recipe):
    return C * 1000 + steps * 100 + shape[2] + (7 if recipe == 'white' else 0)


def case_mask(shape):
    return np.random.default_rng(shape[2]).random(shape) < 0.6
