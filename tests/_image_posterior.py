"""numpy restatement of the image posterior (csrc/image_posterior_kernels.hip), shared by tests/test_image_posterior_host.py and
tests/test_gpu_image_posterior.py, and the inputs both use.

The sampler: `taps` restates axis_tap (csrc/common.h) and the eight corner offsets and weights in float32, operation by
operation; `sample32` accumulates the eight products in float32 in the kernel's order (z, y, x), `sample64` gathers the same
taps in float64.  The fold: `welford32` is the kernel's recurrence in float32 numpy, `two_pass` the float64 mean / variance /
min / max it is held against.  `finalize_np` and `summary_np` restate the finalize from a stored state and stored maps.

The band.  VAR_BAND and MEAN_BAND are the worst error of welford32 itself against two_pass over exactly the record sets of the
GPU test of several steps (STEP_SHAPES x STEP_CHAINS x 1 .. STEP_COUNT steps, `step_case`), measured by
test_image_posterior_host.py::test_restatement_band, which prints them and holds the stored values to the measured ones.  The
variance error is in units of max|x|^2, the mean error in units of the bound 5 K 2^-24 max|x| of K records.  The GPU test
gives the device 4 x VAR_BAND: it contracts m2 + d * (x - mean) into one FMA, the restatement rounds twice.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24

STEP_SHAPES = [(5, 7, 9), (17, 16, 65), (3, 37, 70)]
STEP_CHAINS = [1, 2, 3]
STEP_COUNT = 5
STEP_VOLUMES = 2
# measured by test_restatement_band (printed there): the worst |var32 - var64| / max|x|^2 and the worst |mean32 - mean64| /
# (5 K 2^-24 max|x|) of the float32 recurrence over the record sets of step_case
VAR_BAND = 7.7e-8    # measured 7.6132e-08
MEAN_BAND = 0.089    # measured 0.0884


def mean_bound(K, magnitude):
    """float32 Welford mean of K records of magnitude max|x| (tests/test_gpu_local_similarity.py: 5 K u), scaled by max|x|"""
    return 5.0 * K * U * magnitude


# ---------------------------------------------------------------- inputs
def random_transformation(shape, C, seed, reach=3):
    """(C,3,D,H,W) float32 in [-1,1] coordinates: every coordinate uniform over [-reach, n - 1 + reach] voxels, not on any
    lattice, the two extremes planted on every axis"""
    rng = np.random.default_rng(seed)
    t = np.empty((C, 3, *shape), np.float64)
    for c, n in enumerate((shape[2], shape[1], shape[0])):
        pos = rng.uniform(-reach, n - 1 + reach, (C, *shape))
        where = rng.choice(pos.size, 2, replace=False)
        pos.reshape(-1)[where] = (-reach, n - 1 + reach)
        t[:, c] = -1.0 + pos * (2.0 / (n - 1))
    return t.astype(F32)


def random_volumes(shape, S, seed, lo=-3.0, hi=7.0):
    """(S,1,D,H,W) float32, uniform over [lo, hi): every volume differs"""
    return np.random.default_rng(seed).uniform(lo, hi, (S, 1, *shape)).astype(F32)


def step_case(shape, C):
    """the record set of the several-steps test: STEP_VOLUMES volumes and STEP_COUNT steps of C transformations"""
    seed = 7000 + 10 * STEP_SHAPES.index(tuple(shape)) + C
    return random_volumes(shape, STEP_VOLUMES, seed), [random_transformation(shape, C, seed + 100 * (s + 1)) for s in range(STEP_COUNT)]


# ---------------------------------------------------------------- the sampler
def axis_taps(g, n):
    """axis_tap in float32: -> (i0, i1 int64, w0, w1 float32)"""
    g = np.asarray(g, F32)
    nm1 = F32(n - 1)
    raw = ((g + F32(1.0)) * F32(0.5)) * nm1
    i = np.where(raw <= 0, F32(0.0), np.where(raw >= nm1, nm1, raw)).astype(F32)
    f = np.floor(i)
    i0 = f.astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), ((f + F32(1.0)) - i).astype(F32), (i - f).astype(F32)


def taps(t, shape):
    """transformation (C,3,D,H,W) -> (offsets (C,8,D,H,W) int64 into a flat volume, weights (C,8,D,H,W) float32), the eight
    corners in z, y, x order, the weight (wx * wy) * wz"""
    D, H, W = shape
    x0, x1, wx0, wx1 = axis_taps(t[:, 0], W)
    y0, y1, wy0, wy1 = axis_taps(t[:, 1], H)
    z0, z1, wz0, wz1 = axis_taps(t[:, 2], D)
    off, w = [], []
    for zi, wz in ((z0, wz0), (z1, wz1)):
        for yi, wy in ((y0, wy0), (y1, wy1)):
            for xi, wx in ((x0, wx0), (x1, wx1)):
                off.append((zi * H + yi) * W + xi)
                w.append(((wx * wy).astype(F32) * wz).astype(F32))
    return np.stack(off, 1), np.stack(w, 1)


def sample32(volume, tp):
    """the kernel's sample in float32: acc = acc + v * w, corner by corner -> (C,D,H,W) float32"""
    off, w = tp
    flat = np.asarray(volume, F32).reshape(-1)
    acc = np.zeros(off[:, 0].shape, F32)
    with np.errstate(invalid='ignore'):
        for j in range(8):
            acc = (acc + (flat[off[:, j]] * w[:, j]).astype(F32)).astype(F32)
    return acc


def sample64(volume, tp):
    """the same taps gathered in float64 -> (C,D,H,W) float64"""
    off, w = tp
    flat = np.asarray(volume, np.float64).reshape(-1)
    return sum(flat[off[:, j]] * w[:, j].astype(np.float64) for j in range(8))


def readers(tp, voxel, nonzero=True):
    """(C,D,H,W) bool: the output voxels one of whose taps reads the flat source voxel `voxel` (with a weight != 0)"""
    off, w = tp
    hit = off == voxel
    return (hit & (w != 0)).any(1) if nonzero else hit.any(1)


# ---------------------------------------------------------------- the fold
def welford32(records, state=None, records_before=0):
    """the kernel's fold of records (n, ...) in float32 -> (mean, m2, low, high) float32"""
    mean, m2, low, high = (None,) * 4 if state is None else (np.array(a, F32) for a in state)
    with np.errstate(invalid='ignore'):
        for c, x in enumerate(records):
            x = np.asarray(x, F32)
            k = records_before + c + 1
            if k == 1:
                mean, m2, low, high = x.copy(), np.zeros_like(x), x.copy(), x.copy()
            else:
                d = (x - mean).astype(F32)
                mean = (mean + (d / F32(k)).astype(F32)).astype(F32)
                m2 = (m2 + (d * (x - mean).astype(F32)).astype(F32)).astype(F32)
                low, high = np.fmin(low, x), np.fmax(high, x)
    return mean, m2, low, high


def two_pass(records):
    """float64 two-pass -> (mean, variance with n - 1 (n = 1: 0), min, max)"""
    r = np.asarray(records, np.float64)
    mean = r.mean(0)
    return mean, ((r - mean) ** 2).sum(0) / max(r.shape[0] - 1, 1), r.min(0), r.max(0)


# ---------------------------------------------------------------- the finalize
def finalize_np(mean, m2, low, high, n, reference=None, std_floor=0.0):
    """-> (std, range float32 as the kernel rounds them, z float64 from those stored maps or None); NaN where the mean is not
    finite"""
    mean, m2, low, high = (np.asarray(a, F32) for a in (mean, m2, low, high))
    finite = np.isfinite(mean)
    with np.errstate(invalid='ignore', divide='ignore'):
        std = np.where(finite, np.sqrt((m2 / F32(max(n - 1, 1))).astype(F32)), F32(np.nan)).astype(F32)
        rng = np.where(finite, (high - low).astype(F32), F32(np.nan)).astype(F32)
        z = None if reference is None else z_np(mean, std, reference, std_floor)
    return std, rng, z


def z_np(mean, std, reference, std_floor):
    """z in float64 from the stored float32 maps"""
    mean, std, reference = (np.asarray(a, np.float64) for a in (mean, std, reference))
    with np.errstate(invalid='ignore', divide='ignore'):
        z = (reference - mean) / np.sqrt(std * std + float(np.float32(std_floor)) ** 2)
    return np.where(np.isfinite(mean), z, np.nan)


def summary_np(mean, std, rng, z=None, mask=None):
    """the summary columns from stored maps -> (ints [voxels, non-finite, |z| > 2, |z| > 3], floats [sum mean, sum std, max std,
    max range, sum z^2, max |z|]); without z the last two floats are NaN"""
    m = np.ones(mean.shape, bool) if mask is None else np.asarray(mask) != 0
    finite = np.isfinite(mean) & m
    f = lambda a: np.asarray(a, np.float64)[finite]
    maximum = lambda a: float(a.max()) if a.size else -np.inf
    ints = [int(m.sum()), int((m & ~np.isfinite(mean)).sum()), 0, 0]
    floats = [float(f(mean).sum()), float(f(std).sum()), maximum(f(std)), maximum(f(rng)), np.nan, np.nan]
    if z is not None:
        az = np.abs(f(z))
        az = az[~np.isnan(az)]
        ints[2], ints[3] = int((az > 2).sum()), int((az > 3).sum())
        floats[4], floats[5] = float((az * az).sum()), maximum(az)
    return ints, floats


# ---------------------------------------------------------------- refusals of the C ABI
I32MAX = 2 ** 31 - 1
WS = 1024 * (4 + 6) * 8  # IRS_IMAGE_POSTERIOR_WS_BYTES


def abi_refusals(P):
    """(entry point, arguments that pass with `P` for every pointer, [(case id, replaced arguments, message)]) of the two entry
    points: every refusal include/irsgmcmc.h states"""
    dims = dict(D=4, H=5, W=6)
    update = dict(volumes=P, S=2, transformation=P, C=2, **dims, mean=P, m2=P, low=P, high=P, records_before=0, stream=None)
    finalize = dict(mean=P, m2=P, low=P, high=P, **dims, n=3, reference=P, std_floor=0.5, mask=None, std_out=P, range_out=P, z_out=P,
                    isummary=P, fsummary=P, ws=P, ws_bytes=WS, stream=None)
    bad = 'bad arguments'
    u = [(f'{k}=null', {k: None}, bad) for k in ('volumes', 'transformation', 'mean', 'm2', 'low', 'high')]
    u += [('S=0', dict(S=0), 'S = 0 volumes, 1..8'), ('S=9', dict(S=9), 'S = 9 volumes, 1..8'), ('C=0', dict(C=0), bad),
          ('C=9', dict(C=9), 'C = 9 chains, 1..8'), ('D=1', dict(D=1), bad), ('H=1', dict(H=1), bad), ('W=1', dict(W=1), bad),
          ('W=0', dict(W=0), bad), ('voxels=2^30', dict(D=1024, H=1024, W=1024), bad),
          ('grid-z', dict(D=40000, H=2, W=2, S=5), 'dims (40000, 2, 2) x 5 volumes exceed the launch grid'),
          ('records=-1', dict(records_before=-1), 'records_before = -1 < 0'),
          ('records=ceiling', dict(records_before=I32MAX - 1), f'{I32MAX - 1} records + 2 chains overflow the int32 record count')]
    f = [(f'{k}=null', {k: None}, bad) for k in ('mean', 'm2', 'low', 'high', 'std_out', 'range_out', 'isummary', 'fsummary', 'ws')]
    f += [('D=1', dict(D=1), bad), ('voxels=2^30', dict(D=1024, H=1024, W=1024), bad),
          ('n=0', dict(n=0), 'n = 0 records, at least 1 needed'), ('n=-3', dict(n=-3), 'n = -3 records, at least 1 needed'),
          ('z_out-alone', dict(reference=None), 'reference and z_out go together, one of them is NULL'),
          ('reference-alone', dict(z_out=None), 'reference and z_out go together, one of them is NULL'),
          ('floor=-1', dict(std_floor=-1.0), 'std_floor = -1, a finite value >= 0 needed'),
          ('floor=nan', dict(std_floor=float('nan')), 'std_floor = nan, a finite value >= 0 needed'),
          ('floor=inf', dict(std_floor=float('inf')), 'std_floor = inf, a finite value >= 0 needed'),
          ('ws-1', dict(ws_bytes=WS - 1), f'workspace of {WS - 1} bytes, {WS} needed (IRS_IMAGE_POSTERIOR_WS_BYTES)')]
    return [('irs_image_posterior_update', update, u), ('irs_image_posterior_finalize', finalize, f)]


def abi_call(lib, fn, good, replaced):
    """-> (return code, irs_last_error()) of one call"""
    args = dict(good)
    args.update(replaced)
    rc = getattr(lib, fn)(*args.values())
    return rc, lib.irs_last_error().decode()
