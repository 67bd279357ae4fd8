"""numpy float64 restatement of the affine pre-alignment operators (include/irsgmcmc.h, "Affine pre-alignment"), written from the
header's words alone: it shares no code with ir_sgmcmc_amd/affine.py or the HIP path.  numpy rounds every operation once and
fuses none, so a term formed in the documented order is the device's term bit for bit; only the order of the SUM differs.

With `exact=True` every array is int64 (integer images, integer maps, odd extents): the sums are then exact integers.
"""
import numpy as np

PAIRS3 = [(i, j) for i in range(3) for j in range(i, 3)]
PAIRS4 = [(a, b) for a in range(4) for b in range(a, 4)]


def _axes(p):
    """parameter index -> (which g, which kt)"""
    return (p // 3, p % 3) if p < 9 else (p - 9, 3)


def centred_index(dims, dtype=np.float64):
    D, H, W = dims
    k = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    if dtype == np.int64:
        assert all(n % 2 == 1 for n in dims), 'the exact case needs an integer centre'
        c = [(n - 1) // 2 for n in dims]
    else:
        c = [(n - 1) / 2.0 for n in dims]
    return [k[a].astype(dtype) - c[a] for a in range(3)], c


def mapped(lin, shift, dims, dtype=np.float64):
    """p = c + shift + lin (k - c), the row dot product left to right, then + shift, then + c -> ([p0, p1, p2], d)"""
    d, c = centred_index(dims, dtype)
    p = [(((lin[a][0] * d[0] + lin[a][1] * d[1]) + lin[a][2] * d[2]) + shift[a]) + c[a] for a in range(3)]
    return p, d


def normal_equations(fixed, moving, mask, lin, shift, exact=False):
    """-> {'sums': the 94 values, 'abs': the sum of |term| per value, 'terms': N} (float64, or int64 when exact)"""
    dtype = np.int64 if exact else np.float64
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    dims = fixed.shape
    lin, shift = np.asarray(lin, dtype=dtype), np.asarray(shift, dtype=dtype)
    p, d = mapped(lin, shift, dims, dtype)
    masked = np.ones(dims, bool) if mask is None else np.asarray(mask).astype(bool)
    inside = np.ones(dims, bool)
    for a in range(3):
        inside &= (p[a] >= 0) & (p[a] <= dims[a] - 1)
    sel = masked & inside
    n_outside = int((masked & ~inside).sum())
    i0, w = [], []
    for a in range(3):
        pa = p[a][sel]
        ia = np.minimum(np.floor(pa).astype(np.int64), dims[a] - 2)
        i0.append(ia)
        w.append(pa - ia.astype(dtype))
    f = fixed[sel]
    t32 = [[[moving[i0[0] + a, i0[1] + b, i0[2] + c] for c in range(2)] for b in range(2)] for a in range(2)]
    finite = np.isfinite(f)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                finite &= np.isfinite(t32[a][b][c])
    n_nonfinite = int((~finite).sum())
    t = [[[t32[a][b][c][finite].astype(dtype) for c in range(2)] for b in range(2)] for a in range(2)]
    f = f[finite].astype(dtype)
    w = [wa[finite] for wa in w]
    kt = [d[a][sel][finite] for a in range(3)] + [np.ones(int(finite.sum()), dtype)]
    one = dtype(1)
    wz, wy, wx = ([one - wa, wa] for wa in w)
    m = np.zeros(len(f), dtype)
    g = [np.zeros(len(f), dtype) for _ in range(3)]
    for a in range(2):
        for b in range(2):
            wzy = wz[a] * wy[b]
            for c in range(2):
                m = m + (wzy * wx[c]) * t[a][b][c]
            g[0] = g[0] + (wy[a] * wx[b]) * (t[1][a][b] - t[0][a][b])
            g[1] = g[1] + (wz[a] * wx[b]) * (t[a][1][b] - t[a][0][b])
            g[2] = g[2] + wzy * (t[a][b][1] - t[a][b][0])
    r = m - f
    gg = {ij: g[ij[0]] * g[ij[1]] for ij in PAIRS3}
    kk = {ab: kt[ab[0]] * kt[ab[1]] for ab in PAIRS4}
    sums, absum = [], []

    def add(term):
        sums.append(term.sum())
        absum.append(np.abs(term).sum())

    for pi in range(12):
        for qi in range(pi, 12):
            (gp, kp), (gq, kq) = _axes(pi), _axes(qi)
            add(gg[(min(gp, gq), max(gp, gq))] * kk[(min(kp, kq), max(kp, kq))])
    gr = [g[a] * r for a in range(3)]
    for pi in range(12):
        ga, kb = _axes(pi)
        add(gr[ga] * kt[kb])
    add(r * r)
    n = len(f)
    for count in (n, n_outside, n_nonfinite):
        sums.append(count)
        absum.append(count)
    return {'sums': np.array(sums, dtype=dtype), 'abs': np.array(absum, dtype=dtype), 'terms': n}


def as_dict(sums):
    """the 94 values -> H (12,12), b, ssd, n, n_outside, n_nonfinite as the package's wrapper returns them"""
    v = np.asarray(sums, dtype=np.float64)
    H = np.zeros((12, 12))
    it = 0
    for pi in range(12):
        for qi in range(pi, 12):
            H[pi, qi] = H[qi, pi] = v[it]
            it += 1
    return {'H': H, 'b': v[78:90].copy(), 'ssd': float(v[90]), 'n': int(v[91]), 'n_outside': int(v[92]), 'n_nonfinite': int(v[93])}


def normal_eq_function(fixed, moving, mask, lin, shift):
    """the signature affine.register passes to its operator; takes torch CPU tensors or arrays of any leading 1-dimensions"""
    to3 = lambda x: None if x is None else np.asarray(x).reshape(np.asarray(x).shape[-3:])
    return as_dict(normal_equations(to3(fixed), to3(moving), to3(mask), lin, shift)['sums'])


def transformation(lin, shift, dims):
    """(1,3,D,H,W) float32: 2 p_a / (n_a - 1) - 1 in double, rounded once; component 0 the last axis"""
    p, _ = mapped(np.asarray(lin, np.float64), np.asarray(shift, np.float64), dims)
    return np.stack([((2.0 * p[a]) / float(dims[a] - 1) - 1.0).astype(np.float32) for a in (2, 1, 0)])[None]


def compose(t, lin, shift):
    """t (C,3,D,H,W) float32 in [-1,1] -> (total transformation, total displacement in voxels), float32"""
    t = np.asarray(t)
    dims = t.shape[2:]
    lin, shift = np.asarray(lin, np.float64), np.asarray(shift, np.float64)
    k = np.meshgrid(*[np.arange(n) for n in dims], indexing='ij')
    total_t, total_d = np.empty_like(t), np.empty_like(t)
    for ch in range(t.shape[0]):
        d = []
        for a in range(3):
            g = t[ch, 2 - a].astype(np.float64)
            d.append(((g + 1.0) * 0.5) * float(dims[a] - 1) - (dims[a] - 1) / 2.0)
        for a in range(3):
            q = (((lin[a][0] * d[0] + lin[a][1] * d[1]) + lin[a][2] * d[2]) + shift[a]) + (dims[a] - 1) / 2.0
            total_t[ch, 2 - a] = ((2.0 * q) / float(dims[a] - 1) - 1.0).astype(np.float32)
            total_d[ch, 2 - a] = (q - k[a].astype(np.float64)).astype(np.float32)
    return total_t, total_d


# ---------------------------------------------------------------- the analytic pair
def rodrigues(omega):
    w = np.asarray(omega, np.float64)
    angle = np.linalg.norm(w)
    if angle == 0:
        return np.eye(3)
    x, y, z = w / angle
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def blob_function(dims, seed=0, count=12):
    """a sum of `count` Gaussian blobs with centres in the middle half of the grid and widths 0.08 .. 0.16 of the extent ->
    callable on index coordinates (..., 3)"""
    rng = np.random.default_rng(seed)
    n = np.asarray(dims, np.float64)
    centres = (0.25 + 0.5 * rng.random((count, 3))) * (n - 1)
    widths = (0.08 + 0.08 * rng.random((count, 1))) * n
    amps = 0.5 + rng.random(count)

    def f(q):
        out = np.zeros(q.shape[:-1])
        for mu, s, a in zip(centres, widths, amps):
            out += a * np.exp(-(((q - mu) / s) ** 2).sum(-1) / 2.0)
        return out

    return f


def analytic_pair(dims, lin, shift, seed=0):
    """fixed F(k), moving M(q) = F(A^-1 q) with A: k -> c + shift + lin (k - c), so that M(A k) = F(k) exactly and no
    interpolation enters the truth; mask: the central box inset by n / 6.  float32 images, bool mask."""
    f = blob_function(dims, seed)
    c = (np.asarray(dims, np.float64) - 1) / 2.0
    k = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing='ij'), -1)
    back = (k - c - np.asarray(shift, np.float64)) @ np.linalg.inv(np.asarray(lin, np.float64)).T + c
    mask = np.zeros(dims, bool)
    inset = [n // 6 for n in dims]
    mask[inset[0]:dims[0] - inset[0], inset[1]:dims[1] - inset[1], inset[2]:dims[2] - inset[2]] = True
    return f(k).astype(np.float32), f(back).astype(np.float32), mask


def map_error(lin, shift, true_lin, true_shift, mask):
    """the largest distance, in voxels, between p under the two maps over the masked voxels"""
    dims = mask.shape
    c = (np.asarray(dims, np.float64) - 1) / 2.0
    d = np.stack(np.nonzero(mask), -1).astype(np.float64) - c
    diff = d @ (np.asarray(lin) - np.asarray(true_lin)).T + (np.asarray(shift) - np.asarray(true_shift))
    return float(np.linalg.norm(diff, axis=1).max())


RIGID_CASE = {'dims': (24, 24, 24), 'omega': (0.06, -0.05, 0.087), 'shift': (1.5, -2.0, 1.0)}


def affine_case():
    """32^3: a small rotation times diag(1.05, 0.96, 1.03) plus shears of 0.01 .. 0.03, shift (-1, 1.5, 0.5)"""
    shear = np.array([[0.0, 0.02, -0.01], [0.03, 0.0, 0.015], [-0.02, 0.01, 0.0]])
    lin = rodrigues((0.04, -0.03, 0.05)) @ np.diag([1.05, 0.96, 1.03]) + shear
    return {'dims': (32, 32, 32), 'lin': lin, 'shift': np.array([-1.0, 1.5, 0.5])}
