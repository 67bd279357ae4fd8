"""numpy restatement of the posterior principal modes ("Displacement modes"), the input recipes, the bounds
and the checks, shared by the host and the GPU tests.

Gram matrix.  G[c,i,j] = sum over the masked voxels of x_i x_j per channel.  Every product of two float32 values is exact in
float64, so the only error of a float64 evaluation is the k - 1 additions of the k masked voxels, in whatever order:
    |G - exact| <= gamma_{k-1} sum |x_i x_j|,   gamma_m = m w / (1 - m w),  w = 2^-53.
The reference is math.fsum of the exact products, the correctly rounded exact sum: |fsum - exact| <= w |exact| <= w sum |x_i x_j|.
Together |G - fsum| <= gamma_k sum |x_i x_j| (gamma_{k-1} + w <= gamma_k), the bound of the definitions, with no measured margin.
Records of small dyadic values (integers in -8 .. 8 times 2^-4) make every partial sum exact: any order gives the same bits, and
the comparison is bit for bit.

Projection.  `project_np` restates the kernel in its operation order (numpy float64 rounds every operation once and fuses
nothing): per voxel and channel, in record order from zero, S += x_i, Q += x_i x_i, a_m += coeff[m,i] x_i (product rounded, then
the sum); mean = float32(S / n), modes = float32(a_m).  Those two are compared bit for bit.  The explained ratio is compared with
a float64 reference that forms the variance from centred data (`explained_ref`), within the forward bound B below, derived with
w = 2^-53, u = 2^-24 and n only.  A = sum_i |x_i|, Q* = sum_i x_i^2 per channel; s2_c the squared scale.
  variance.  The computed S is sum x_i (1 + theta_{n-1}), so |S^2 - S*^2| <= gamma_{2n-2} A^2; the square, the division by n, the
    subtraction and the division by n - 1 add four roundings, and Q carries gamma_{n-1} and the last two of those:
        d[(n - 1) var_c] <= gamma_{n+1} Q* + gamma_{2n+2} A^2 / n =: Dv_c.
  denominator.  den = sum_c s2_c var_c, three products and two additions:
        dden <= (1 + gamma_3) sum_c s2_c Dv_c / (n - 1) + gamma_3 sum_c s2_c |var_c|.
  numerator.  a_m is n rounded products and n - 1 rounded additions: |a_m - a_m*| <= gamma_n sum_i |coeff[m,i] x_i| =: da_m.  The
    restatement and the kernel hold the same a_m bit for bit, but the reference below forms a_m with numpy's dot product, in
    another order, so da_m stays.  The squares, their sum over M modes, the scale and the sum over three channels are at most
    M + 4 more roundings (a fused multiply-add drops one and never adds one):
        dnum <= (1 + gamma_{M+4}) sum_c s2_c sum_m (2 |a_m| da_m + da_m^2) + gamma_{M+4} num.
  ratio.  |num / den - num* / den*| <= (dnum + e* dden) / (den* - dden) where dden < den*, and the division and the float32
    store add (w + u) e*.  B = FACTOR (that sum), FACTOR = 2 for the reference's own float64 error -- bounded by the same
    expressions, its centred variance by less -- and the second-order terms left out.  Voxels with FACTOR dden > den* / 2 are
    left out of the comparison (the textbook variance has cancelled there); the recipes have none, which the tests assert.
  A voxel whose records are all zero has S = Q = a_m = 0 exactly: den == 0 and the value is exactly 0.  A voxel whose records
  share one small dyadic value has every intermediate exact (n x, n x^2 and (n x)^2 fit 53 bits), so den == 0 there too.

Host algebra.  `decompose_np` restates modes.modes_decompose; `svd_np` is the independent route: the singular values of the
centred, scaled, masked data matrix give lambda_m = sigma_m^2 / (n - 1) and its right singular vectors times sigma_m /
sqrt(n - 1) the mode fields, up to the sign rule.

Planted modes (`planted_records`).  Three orthonormal fields psi_k (masked, scaled inner product), scores the columns of the QR
of a centred random n x 3 matrix times (4, 2, 1) sqrt(n - 1), a constant offset and white noise of 0.05 of the smallest
amplitude per unit-norm direction.  The sample covariance of the records is then C = P + N with P = sum_k a_k^2 psi_k psi_k^T
exactly of eigenvalues 16 : 4 : 1 and N the noise terms; |N|_2 is computed in the test from the (n + 3) x (n + 3) Gram matrix of
[Xc^T / sqrt(n - 1), Psi diag(a)] (the non-zero eigenvalues of B J B^T are those of J B^T B, J = diag(I_n, -I_3)).
  eigenvalues (Weyl): |lambda_m - a_m^2| <= |N|_2 + eG, eG = |dG|_F / (n - 1) the Gram bound above carried through the scale.
  modes (Davis-Kahan, Yu, Wang and Samworth 2015): sin angle(phi_m, psi_m) <= 2 (|N|_2 + eG) / delta_m + 2^-20, delta_m the gap
  of a_m^2 to its neighbours among (16, 4, 1, 0) a_3^2; 2^-20 covers the float32 storage of the 3 V components.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
W = 2.0 ** -53
FACTOR = 2.0

SHAPES = ((2, 2, 3), (5, 6, 7), (16, 12, 20), (24, 20, 28))


def gamma(m, w=W):
    return m * w / (1 - m * w)


def default_scale(shape):
    D, H, Wd = shape
    return ((Wd - 1) / 2, (H - 1) / 2, (D - 1) / 2)


# ---------------------------------------------------------------- masks and records
MASKS = ('none', 'full', 'random', 'empty', 'one')


def make_mask(kind, shape):
    """-> bool volume or None"""
    if kind == 'none':
        return None
    if kind == 'full':
        return np.ones(shape, dtype=bool)
    if kind == 'empty':
        return np.zeros(shape, dtype=bool)
    if kind == 'one':
        m = np.zeros(shape, dtype=bool)
        m[shape[0] - 1, shape[1] // 2, 1] = True
        return m
    return np.random.default_rng(shape[2]).random(shape) < 0.6


def dyadic_records(n, shape, seed):
    """integers in -8 .. 8 times 2^-4: every Gram sum is exact in double"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-8, 9, size=(n, 3) + tuple(shape)) / 16.0).astype(np.float32)


def random_records(n, shape, seed):
    """a smooth-free recipe: a per-voxel offset plus per-record noise, normalised coordinates of a few voxels"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, size=(1, 3) + tuple(shape))
    x = base + 0.3 * rng.standard_normal(size=(n, 3) + tuple(shape))
    return (x * 0.05).astype(np.float32)


# (shape, the records of the successive appends, mask): n from 1 to 40, every chain count, n_before = 0, values that are no
# multiple of the tile of 8 stored records, and a last append that ends exactly at the cap (cap = the sum)
GRAM_CASES = (
    ((2, 2, 3), (1,), 'none'),
    ((2, 2, 3), (2, 1, 3), 'one'),
    ((5, 6, 7), (3, 3, 3, 1), 'random'),
    ((5, 6, 7), (8, 8, 8, 8, 8), 'none'),
    ((16, 12, 20), (2, 2, 2, 2, 2, 1), 'full'),
    ((16, 12, 20), (1, 2, 3, 8, 3), 'empty'),
    ((24, 20, 28), (8, 3, 2, 8, 8, 8, 3), 'random'),
    ((24, 20, 28), (2, 2, 2), 'none'),
)


def gram_case_seed(shape, appends, family):
    return shape[2] * 100 + sum(appends) + (5000 if family == 'random' else 0)


@functools.lru_cache(maxsize=None)
def gram_case(index, family):
    """-> (records (n,3,D,H,W) float32, mask or None, reference (3,n,n) float64, bound (3,n,n)): dyadic -> the exact float64
    matrix and a bound of 0; random -> math.fsum of the exact products and gamma_k sum |x_i x_j|.  Read-only."""
    shape, appends, kind = GRAM_CASES[index]
    n = sum(appends)
    records = (dyadic_records if family == 'dyadic' else random_records)(n, shape, gram_case_seed(shape, appends, family))
    mask = make_mask(kind, shape)
    ref, bound = gram_reference(records, mask, exact=family == 'dyadic')
    for a in (records, ref, bound):
        a.setflags(write=False)
    return records, mask, ref, bound


def gram_np(records, mask=None):
    """the float64 evaluation: exact products, numpy's own summation order"""
    n = records.shape[0]
    x = records.reshape(n, 3, -1).astype(np.float64)
    if mask is not None:
        x = x[:, :, np.asarray(mask).reshape(-1)]
    return np.einsum('icv,jcv->cij', x, x)


def gram_reference(records, mask=None, exact=False):
    """-> (G (3,n,n), bound (3,n,n)).  exact: the float64 matrix of records whose sums are exact, bound 0.  Otherwise math.fsum
    of the exact products per entry and gamma_k sum |x_i x_j|, k the masked voxels."""
    n = records.shape[0]
    x = records.reshape(n, 3, -1).astype(np.float64)
    if mask is not None:
        x = x[:, :, np.asarray(mask).reshape(-1)]
    k = x.shape[2]
    if exact:
        return gram_np(records, mask), np.zeros((3, n, n))
    G, S = np.zeros((3, n, n)), np.zeros((3, n, n))
    for c in range(3):
        for i in range(n):
            for j in range(i + 1):
                p = x[i, c] * x[j, c]
                G[c, i, j] = G[c, j, i] = math.fsum(p)
                S[c, i, j] = S[c, j, i] = math.fsum(np.abs(p))
    return G, gamma(k) * S * (1 + 2 * W)  # (the sum of absolute values is itself a rounded number)


# ---------------------------------------------------------------- host algebra
def decompose_np(G3, scale, mask_voxels):
    """the definitions, in numpy float64 -> (lam (n-1,) descending and clamped, vectors (n, n-1) with the sign rule, Gc)"""
    G3 = np.asarray(G3, dtype=np.float64)
    n = G3.shape[1]
    s = np.asarray(scale, dtype=np.float64)
    G = s[0] * s[0] * G3[0] + s[1] * s[1] * G3[1] + s[2] * s[2] * G3[2]
    H = np.eye(n) - np.full((n, n), 1.0 / n)
    Gc = H @ G @ H / (n - 1)
    Gc = 0.5 * (Gc + Gc.T)
    w, Uv = np.linalg.eigh(Gc)
    order = np.argsort(-w, kind='stable')[:n - 1]
    lam, Uv = np.maximum(w[order], 0.0), Uv[:, order]
    for m in range(Uv.shape[1]):
        if Uv[np.argmax(np.abs(Uv[:, m])), m] < 0:
            Uv[:, m] = -Uv[:, m]
    return lam, Uv, Gc


def data_matrix(records, scale, mask=None):
    """(n, 3 k) float64: the records scaled per channel, the masked voxels only"""
    n = records.shape[0]
    x = records.reshape(n, 3, -1).astype(np.float64) * np.asarray(scale, dtype=np.float64).reshape(1, 3, 1)
    if mask is not None:
        x = x[:, :, np.asarray(mask).reshape(-1)]
    return x.reshape(n, -1)


def svd_np(records, scale, mask=None):
    """-> (lambda (min(n, 3k),), fields (., 3k): right singular vectors times sigma / sqrt(n - 1), the centred data matrix)"""
    X = data_matrix(records, scale, mask)
    Xc = X - X.mean(axis=0, keepdims=True)
    _, sv, Vt = np.linalg.svd(Xc, full_matrices=False)
    n = X.shape[0]
    return sv ** 2 / (n - 1), Vt * (sv / math.sqrt(n - 1))[:, None], Xc


def split_rhat_np(series):
    """(C, N) -> scalar split-R-hat by the formula of ops.split_rhat / utils.calc_split_rhat"""
    C, N = series.shape
    h = N // 2
    halves = np.concatenate([series[:, :h], series[:, N - h:]], axis=0)
    means = halves.mean(axis=1)
    Wv = np.mean(((halves - means[:, None]) ** 2).sum(axis=1) / (h - 1))
    B = means.var(ddof=1)
    if Wv == 0:
        return 1.0 if B == 0 else math.inf
    return math.sqrt(((h - 1) / h * Wv + B) / Wv)


# ---------------------------------------------------------------- projection
def project_np(records, coeff, scale, dtype=np.float64):
    """the kernel's operation order in numpy `dtype` (float64: the restatement; every operation rounded once, none fused) ->
    dict: mean (3,...) float32, modes (M,3,...) float32, explained (...) float32, and the float64 internals S, Q, a, num, den"""
    records = np.asarray(records, dtype=np.float32)
    coeff = np.asarray(coeff, dtype=np.float64)
    n, shape = records.shape[0], records.shape[2:]
    M = coeff.shape[0]
    s2 = np.asarray(scale, dtype=np.float64) ** 2
    S = np.zeros((3,) + shape, dtype=dtype)
    Q = np.zeros((3,) + shape, dtype=dtype)
    a = np.zeros((M, 3) + shape, dtype=dtype)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i in range(n):
            x = records[i].astype(dtype)
            S = S + x
            Q = Q + x * x
            for m in range(M):
                a[m] = a[m] + dtype(coeff[m, i]) * x
        mean = (S / dtype(n)).astype(np.float32)
        num = np.zeros(shape, dtype=dtype)
        den = np.zeros(shape, dtype=dtype)
        for c in range(3):
            q = np.zeros(shape, dtype=dtype)
            for m in range(M):
                q = q + a[m, c] * a[m, c]
            num = num + dtype(s2[c]) * q
            if n > 1:
                var = (Q[c] - (S[c] * S[c]) / dtype(n)) / dtype(n - 1)
                den = den + dtype(s2[c]) * var
        zero = (den == 0) | (n < 2)
        explained = np.where(zero, 0.0, num / np.where(zero, 1.0, den)).astype(np.float32)
    return {'mean': mean, 'modes': a.astype(np.float32), 'explained': explained, 'S': S, 'Q': Q, 'a': a, 'num': num, 'den': den}


def explained_ref(records, coeff, scale):
    """float64 reference of the explained ratio with the variance from centred data, and the bound B of the module docstring ->
    (e (...), B (...), held (...): where the bound applies)"""
    x = np.asarray(records, dtype=np.float32).astype(np.float64)
    coeff = np.asarray(coeff, dtype=np.float64)
    n, shape = x.shape[0], x.shape[2:]
    M = coeff.shape[0]
    s2 = (np.asarray(scale, dtype=np.float64) ** 2).reshape(3, *([1] * len(shape)))
    if n < 2:
        zeros = np.zeros(shape)
        return zeros, zeros, np.ones(shape, dtype=bool)
    xc = x - x.mean(axis=0, keepdims=True)
    var = (xc ** 2).sum(axis=0) / (n - 1)
    a = np.tensordot(coeff, x, axes=(1, 0))                 # (M,3,...)
    den = (s2 * var).sum(axis=0)
    num = (s2 * (a ** 2).sum(axis=0)).sum(axis=0)
    A = np.abs(x).sum(axis=0)
    Qs = (x ** 2).sum(axis=0)
    Dv = gamma(n + 1) * Qs + gamma(2 * n + 2) * A ** 2 / n
    dden = (1 + gamma(3)) * (s2 * Dv).sum(axis=0) / (n - 1) + gamma(3) * (s2 * np.abs(var)).sum(axis=0)
    da = gamma(n) * np.tensordot(np.abs(coeff), np.abs(x), axes=(1, 0))
    dnum = (1 + gamma(M + 4)) * (s2 * (2 * np.abs(a) * da + da ** 2).sum(axis=0)).sum(axis=0) + gamma(M + 4) * num
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
        held = (den == 0) | (FACTOR * dden <= 0.5 * den)
        B = np.where(den > 0, FACTOR * ((dnum + e * dden) / np.where(held & (den > 0), den - dden, 1.0) + (W + U) * e), 0.0)
    return e, B, held


# n, M, coefficient recipe of the projection cases; every shape of SHAPES takes each
PROJECT_CASES = ((1, 1, 'dense'), (2, 1, 'eigen'), (2, 3, 'dense'), (7, 3, 'eigen'), (7, 8, 'dense'), (40, 8, 'eigen'), (40, 16, 'dense'),
                 (40, 16, 'eigen'))


@functools.lru_cache(maxsize=None)
def project_case(shape, n, M, recipe):
    """-> (records, coeff (M,n) float64, scale, restatement dict, (e, B, held)).  'eigen': the 1-sigma coefficients of the
    records' own modes (rows past n - 1: zero); 'dense': random"""
    seed = shape[2] * 1000 + n * 20 + M + (1 if recipe == 'dense' else 0)
    records = random_records(n, shape, seed)
    scale = default_scale(shape)
    rng = np.random.default_rng(seed + 1)
    if recipe == 'dense' or n < 2:
        coeff = rng.standard_normal((M, n))
    else:
        lam, Uv, _ = decompose_np(gram_np(records), scale, int(np.prod(shape)))
        H = np.eye(n) - np.full((n, n), 1.0 / n)
        coeff = np.zeros((M, n))
        K = min(M, n - 1)
        coeff[:K] = (H @ Uv[:, :K]).T / math.sqrt(n - 1)
    coeff = np.ascontiguousarray(coeff)
    out = project_np(records, coeff, scale)
    ref = explained_ref(records, coeff, scale)
    records.setflags(write=False)
    coeff.setflags(write=False)
    return records, coeff, scale, out, ref


def check_explained(explained, ref):
    """hold a float32 explained map to (e, B, held); prints, then asserts -> worst error over bound"""
    e, B, held = ref
    got = np.asarray(explained).astype(np.float64)
    assert np.asarray(explained).dtype == np.float32
    assert held.all(), float((~held).mean())  # a condition on the inputs
    err = np.abs(got - e)
    zero = B == 0
    assert (err[zero] == 0).all()
    ratio = float((err[~zero] / B[~zero]).max()) if (~zero).any() else 0.0
    print({'explained: worst error': float(err.max()) if err.size else 0.0, 'worst error / bound': ratio})
    assert ratio <= 1.0
    return ratio


# ---------------------------------------------------------------- planted modes
AMPLITUDES = (4.0, 2.0, 1.0)
NOISE = 0.05
PLANTED_CASES = ((5, 1), (6, 2), (12, 3), (24, 2), (40, 1), (12, 2), (6, 3))  # n, C


def planted_records(n, shape, seed, mask=None):
    """-> (records (n,3,D,H,W) float32 in normalised coordinates, psi (3, 3 V) orthonormal in the masked scaled inner product
    (zero outside the mask), scale).  Amplitudes in voxel units: mode k has norm AMPLITUDES[k] in that inner product."""
    rng = np.random.default_rng(seed)
    V = int(np.prod(shape))
    scale = np.asarray(default_scale(shape))
    m = np.ones(V, dtype=bool) if mask is None else np.asarray(mask).reshape(-1)
    raw = rng.standard_normal((3, 3, V)) * m
    psi, _ = np.linalg.qr(raw.reshape(3, -1).T)
    psi = psi.T                                              # (3, 3V), orthonormal rows, voxel units
    Z = rng.standard_normal((n, 3))
    Z -= Z.mean(axis=0, keepdims=True)
    Qm, _ = np.linalg.qr(Z)                                  # centred orthonormal columns
    scores = Qm * np.asarray(AMPLITUDES) * math.sqrt(n - 1)
    noise = NOISE * AMPLITUDES[-1] * rng.standard_normal((n, 3 * V)) / math.sqrt(3 * V) * math.sqrt(n - 1) / math.sqrt(n)
    offset = 0.5 * rng.standard_normal((1, 3 * V)) / math.sqrt(3 * V)
    fields = scores @ psi + noise + offset                   # voxel units
    records = (fields.reshape(n, 3, V) / scale.reshape(1, 3, 1)).reshape((n, 3) + tuple(shape)).astype(np.float32)
    return records, psi, tuple(scale)


def planted_perturbation(records, psi, scale, mask=None):
    """|N|_2 of C = P + N (module docstring), from the float32 records as stored"""
    X = data_matrix(records, scale, mask)
    n = X.shape[0]
    Xc = X - X.mean(axis=0, keepdims=True)
    P = psi.reshape(3, 3, -1)
    if mask is not None:
        P = P[:, :, np.asarray(mask).reshape(-1)]
    P = P.reshape(3, -1) * np.asarray(AMPLITUDES).reshape(3, 1)
    B = np.concatenate([Xc / math.sqrt(n - 1), P], axis=0)   # (n + 3, 3k): the rows of B^T
    J = np.diag(np.concatenate([np.ones(n), -np.ones(3)]))
    return float(np.max(np.abs(np.linalg.eigvals(J @ (B @ B.T)))))
