"""Known-transformation validation: are the posterior's error bars right?

Deform an image by a transformation you know, register it, and ask at every voxel how far the posterior mean is from the truth
and whether the truth lies inside the credible region as often as the posterior claims.

 - `simulate_velocity` (host, numpy): a deterministic smooth velocity field in voxels; `known_pair` (device): the moving triple
   made from the FIXED one by the package's own inverse exponential and warps, the dense truth -- the displacement of exp(v*)
   in the unit the recorders receive `output['displacement']` in, voxels of the registration grid -- and the truth's own error
   floor; `read_truth`: a truth from elsewhere, as a legacy `.vtk` vector file.
 - `truth_update`: one recorded step against the truth, one HIP pass for all chains: the per-voxel rank counts `below` and per
   chain the masked error sums (include/irsgmcmc.h: irs_truth_update); `truth_calibrate`: a displacement covariance state against
   the truth, once at the end: error and Mahalanobis maps, PIT and rank histograms, coverage counts, the reliability table and a
   summary (irs_truth_calibrate).  No distribution function is evaluated on the device: `calibration_thresholds` forms the
   thresholds on the host.
 - `calibration_summary`: the derived numbers, on the host in float64.
 - `truth_options` / `truth_metric_names` / the CSV rows of the trainer's option.

The mean of n records is compared with the truth under the PREDICTIVE covariance of one more record: a truth drawn from the law
of the records has d^2 = (mean - t)^T S^-1 (mean - t) distributed as (1 + 1/n) 3 (n - 1) / (n - 3) F(3, n - 3) (Hotelling), not
chi^2_3; `reference: "hotelling"` uses that law for the thresholds and for the expected factor, `"chi2"` the n -> infinity limit.
The records of a chain are autocorrelated, n_eff < n: a scale factor above 1 there can be the Monte-Carlo error of the mean
rather than an under-dispersed posterior.

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import ctypes as C
import hashlib
import math
import numbers

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ops import _call, _check_state, _dims5, _three_positive, _volume_mask

UPDATE_INT_COLUMNS = ('voxels', 'non_finite')
UPDATE_FLOAT_COLUMNS = ('sum_error', 'sum_error2', 'max_error')
SUMMARY_INT_COLUMNS = ('voxels', 'non_finite', 'raised')
SUMMARY_FLOAT_COLUMNS = ('sum_error', 'sum_error2', 'max_error', 'sum_d2', 'max_d2', 'sum_var', 'sum_z_x', 'sum_z_y', 'sum_z_z')
RELIABILITY_STD_RANGE = (0.01, 10.0)  # the default bins of the predicted total std, in the unit of `scale`
REFERENCES = ('hotelling', 'chi2')
SOURCES = ('simulate', 'file')
UNITS = ('voxels', 'mm')
OPTION_KEYS = ('source', 'seed', 'amplitude', 'modes', 'max_wavenumber', 'noise', 'path', 'unit', 'period', 'levels', 'pit_bins',
               'rank_bins', 'reliability_bins', 'std_floor', 'reference', 'save')
SIMULATE_KEYS, FILE_KEYS = ('seed', 'amplitude', 'modes', 'max_wavenumber', 'noise'), ('path', 'unit')
OPTION_DEFAULTS = {'seed': 0, 'amplitude': 2.0, 'modes': 6, 'max_wavenumber': 2, 'noise': 0.0, 'path': None, 'unit': 'voxels',
                   'levels': (0.5, 0.9, 0.95), 'pit_bins': 20, 'rank_bins': 16, 'reliability_bins': 16, 'std_floor': 1e-3,
                   'reference': 'hotelling', 'save': True}
SERIES_COLUMNS = ('record', 'step', 'chain', 'error_mean', 'error_rms', 'error_max', 'voxels', 'non_finite')
MIN_RECORDS = {'hotelling': 6, 'chi2': 2}  # the Hotelling factor needs n - 5 > 0


# ---------------------------------------------------------------- a pair with a known transformation
def simulate_velocity(dims, seed, amplitude, modes=6, max_wavenumber=2):
    """A deterministic smooth velocity field in VOXELS on the host: (3,D,H,W) float32, channels x, y, z as everywhere.

    With xi_z, xi_y, xi_x = linspace(-1, 1, n) of the three axes in float64 and rng = numpy.random.default_rng(seed), drawn in
    this order: k = rng.integers(1, max_wavenumber + 1, size=(3, modes, 3)), phase = rng.uniform(0, 2 pi, size=(3, modes, 3)),
    weight = rng.standard_normal((3, modes)) -- indexed [channel, mode, axis] with the axes in (z, y, x) order --
        v_c = window * sum_m weight[c, m] * prod_a sin(pi * k[c, m, a] * xi_a + phase[c, m, a]),   window = prod_a (1 - xi_a^2),
    so v vanishes on the six boundary faces.  The scaling rule: the float64 field is multiplied by amplitude / max |v| and
    rounded to float32 once; the result is clamped to +-float32(amplitude) and the element that held the largest float64
    magnitude (the first in C order) is set to +-float32(amplitude), so that max |v| over voxels and channels is float32(amplitude)
    exactly (both steps change nothing unless a rounding fell the other way).  amplitude = 0 gives zeros."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 2:
        raise ValueError(f'simulate_velocity: three dims of at least 2, got {dims}')
    if not (isinstance(amplitude, numbers.Real) and math.isfinite(amplitude) and amplitude >= 0):
        raise ValueError(f'simulate_velocity: amplitude must be a finite number >= 0, got {amplitude!r}')
    modes, max_wavenumber = int(modes), int(max_wavenumber)
    if modes < 1 or max_wavenumber < 1:
        raise ValueError(f'simulate_velocity: modes = {modes} and max_wavenumber = {max_wavenumber}, at least 1 each needed')
    rng = np.random.default_rng(seed)
    k = rng.integers(1, max_wavenumber + 1, size=(3, modes, 3))
    phase = rng.uniform(0.0, 2.0 * np.pi, size=(3, modes, 3))
    weight = rng.standard_normal((3, modes))
    xi = [np.linspace(-1.0, 1.0, n) for n in dims]
    shapes = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    window = np.ones(dims)
    for a in range(3):
        window = window * (1.0 - xi[a] ** 2).reshape(shapes[a])
    v = np.zeros((3,) + dims)
    for c in range(3):
        for m in range(modes):
            term = np.full(dims, weight[c, m])
            for a in range(3):
                term = term * np.sin(np.pi * k[c, m, a] * xi[a] + phase[c, m, a]).reshape(shapes[a])
            v[c] += term
        v[c] *= window
    peak = np.abs(v).max()
    if amplitude == 0 or not peak > 0:
        return np.zeros((3,) + dims, dtype=np.float32)
    a32 = np.float32(amplitude)
    out = np.clip((v * (amplitude / peak)).astype(np.float32), -a32, a32)
    at = np.unravel_index(int(np.argmax(np.abs(v))), v.shape)
    out[at] = a32 if v[at] > 0 else -a32
    return out


def known_pair(fixed, v_true, no_steps=12, noise=0.0, seed=0):
    """The moving triple of a pair whose transformation is known.  fixed: {'im' (1,1,D,H,W) float32, 'mask' bool[, 'seg' int16]}
    on the device; v_true (3,D,H,W) float32 in voxels (an array or a tensor).  phi* = exp(v*) and phi*^-1 = exp(-v*) come from
    ops.svf_exp_fwd / ops.svf_exp_inverse with `no_steps`, the entry points the transformation module and the inverse-consistency
    recorder use.  The moving image is the fixed one pulled through phi*^-1 by ops.warp (trilinear) plus, with noise > 0, fresh
    Gaussian noise of that std from a torch generator seeded with `seed` (drawn on the host: the same on every device); mask and
    segmentation go through the nearest-neighbour warp.  So moving o phi* ~ fixed.  A v* that is zero everywhere has exp(v*) = id
    exactly, and the moving triple is then the fixed one bit for bit (no resampling).
    -> (moving dict, truth (3,D,H,W) float32 on the device: the displacement of phi* in voxels, as the transition writes
    output['displacement'], info {'amplitude': max |v*|, 'truth_max': max |truth_c|, 'floor_mean', 'floor_max': mean and max of
    |phi*^-1 o phi* - id| in voxels over the fixed mask (ops.inverse_consistency), 'floor_voxels'}).  An error below the floor
    means nothing: the truth itself is not known better.  One device-to-host read."""
    im = fixed['im']
    if im.dim() != 5 or im.shape[:2] != (1, 1):
        raise L.IrsError(f'known_pair: fixed["im"] must have shape (1,1,D,H,W), got {tuple(im.shape)}')
    D, H, W = im.shape[2:]
    v = torch.as_tensor(np.asarray(v_true.detach().cpu() if torch.is_tensor(v_true) else v_true, dtype=np.float32))
    if tuple(v.shape) != (3, D, H, W):
        raise L.IrsError(f'known_pair: v_true must have shape (3,{D},{H},{W}), got {tuple(v.shape)}')
    if isinstance(noise, bool) or not isinstance(noise, numbers.Real) or not math.isfinite(noise) or noise < 0:
        raise L.IrsError(f'known_pair: noise must be a finite number >= 0, got {noise!r}')
    identity = not bool(v.any())  # on the host
    v = v.to(im.device).unsqueeze(0).contiguous()
    t_fwd, d_fwd, _ = ops.svf_exp_fwd(v, int(no_steps))
    t_inv, d_inv = ops.svf_exp_inverse(v, int(no_steps))
    moving = {}
    for key, vol in fixed.items():
        if key not in ('im', 'mask', 'seg'):
            continue
        moving[key] = vol.clone() if identity else ops.warp(vol.contiguous(), t_inv)
    if noise > 0:
        gen = torch.Generator().manual_seed(int(seed))
        moving['im'] = moving['im'] + (float(noise) * torch.randn(im.shape, generator=gen)).to(im.device)
    mask = fixed.get('mask')
    _, _, isum, fsum = ops.inverse_consistency(t_fwd, d_fwd, d_inv, mask=None if mask is None else mask.bool())
    host = torch.cat([isum.reshape(-1).view(torch.float64), fsum.reshape(-1), v.abs().max().double().reshape(1),
                      d_fwd.abs().max().double().reshape(1)]).cpu()
    voxels, nonfinite = (int(x) for x in host[:2].view(torch.int64))
    finite = voxels - nonfinite
    info = {'amplitude': float(host[5]), 'truth_max': float(host[6]), 'floor_mean': float(host[2]) / finite if finite else math.nan,
            'floor_max': float(host[4]) if finite else math.nan, 'floor_voxels': finite}
    return moving, d_fwd[0].contiguous(), info


def read_truth(path, dims, unit='voxels', spacing=(1.0, 1.0, 1.0)):
    """A truth displacement on the fixed registration grid from a legacy `.vtk` vector file as the package writes its fields
    (utils.imageio.read_vtk_vectors: (3,D,H,W), channels x, y, z) -> (3,D,H,W) float32 on the host, in voxels, the unit of the
    recorded displacement.  unit: "voxels" (taken as it is) or "mm": channel c is divided by spacing[c] (the package saves its own
    fields multiplied by the spacing).  Refuses another grid, another unit and non-finite values."""
    from .utils.imageio import read_vtk_vectors
    if unit not in UNITS:
        raise ValueError(f'read_truth: unit must be one of {list(UNITS)}, got {unit!r}')
    _, file_dims, field = read_vtk_vectors(path)
    dims = tuple(int(d) for d in dims)
    if tuple(file_dims) != dims:
        raise ValueError(f'read_truth: {path} is on a {tuple(file_dims)} grid, the registration grid is {dims}')
    field = np.asarray(field, dtype=np.float32)
    if unit == 'mm':
        sp = np.asarray([float(s) for s in np.asarray(spacing).reshape(-1)][:3], dtype=np.float64)
        if sp.shape != (3,) or not np.all(np.isfinite(sp) & (sp > 0)):
            raise ValueError(f'read_truth: spacing must hold three finite values > 0, got {spacing}')
        field = (field.astype(np.float64) / sp.reshape(3, 1, 1, 1)).astype(np.float32)
    if not np.isfinite(field).all():
        raise ValueError(f'read_truth: {path} holds {int((~np.isfinite(field)).sum())} non-finite values')
    return np.ascontiguousarray(field)


def fingerprint(truth):
    """sha256 of the truth's float32 bytes (a checkpoint resumed on another truth is refused)"""
    arr = np.ascontiguousarray(np.asarray(truth.detach().cpu() if torch.is_tensor(truth) else truth, dtype=np.float32))
    return hashlib.sha256(arr.tobytes()).hexdigest()


# ---------------------------------------------------------------- the two operators
def _truth_state(truth, below, shape):
    _check_state(('truth', truth, (3, *shape), torch.float32), ('below', below, (3, *shape), torch.uint16))


def new_below(dims, device):
    """a fresh (3,D,H,W) uint16 rank-count state"""
    return torch.zeros((3,) + tuple(int(d) for d in dims), device=device, dtype=torch.int16).view(torch.uint16)


class TruthWorkspace:
    """the device workspaces of truth_update and truth_calibrate, allocated once and handed to every call"""

    def __init__(self, device):
        self.update = torch.empty(L.IRS_TRUTH_UPDATE_WS_BYTES, device=device, dtype=torch.uint8)
        self.calibrate = torch.empty(L.IRS_TRUTH_CALIBRATE_WS_BYTES, device=device, dtype=torch.uint8)


def truth_update(displacement, truth, below, records_before, scale=(1.0, 1.0, 1.0), mask=None, out=None, workspace=None):
    """One recorded step against the truth: displacement (C,3,D,H,W) float32, every chain's sample; truth (3,D,H,W) float32 in
    the same unit; below (3,D,H,W) uint16, updated in place: += the number of chains whose component is strictly below the
    truth's (records_before = 0 overwrites it; records_before + C may not exceed IRS_TRUTH_MAX_RECORDS, which is refused before
    any launch); scale: three finite floats > 0; mask (D,H,W) bool / uint8 or None -- the counts ignore it.  -> (ints (C,2) int64
    UPDATE_INT_COLUMNS, floats (C,3) float64 UPDATE_FLOAT_COLUMNS of |scale o (u - truth)| over the mask) on the device.  out: a
    pair of contiguous tensors of those shapes to write into -- rows of a larger series, say.  workspace: a TruthWorkspace
    (allocated here when None).  No host synchronisation (include/irsgmcmc.h: irs_truth_update)."""
    Cn, D, H, W = _dims5(displacement, 3)
    _truth_state(truth, below, (D, H, W))
    records_before = int(records_before)
    if records_before < 0 or records_before + Cn > L.IRS_TRUTH_MAX_RECORDS:
        raise L.IrsError(f'{records_before} + {Cn} records: a uint16 count holds 0..{L.IRS_TRUTH_MAX_RECORDS}')
    mask = _volume_mask(mask, D, H, W)
    sc = _three_positive('scale', scale)
    dev = displacement.device
    if out is None:
        out = (torch.empty((Cn, L.IRS_TRUTH_UPDATE_INTS), device=dev, dtype=torch.int64),
               torch.empty((Cn, L.IRS_TRUTH_UPDATE_FLOATS), device=dev, dtype=torch.float64))
    ints, floats = out
    _check_state(('out[0]', ints, (Cn, L.IRS_TRUTH_UPDATE_INTS), torch.int64),
                 ('out[1]', floats, (Cn, L.IRS_TRUTH_UPDATE_FLOATS), torch.float64))
    ws = (workspace or TruthWorkspace(dev)).update
    _call('irs_truth_update', L.dev_ptr(displacement, torch.float32), Cn, D, H, W, L.dev_ptr(truth, torch.float32),
          L.dev_ptr(below, torch.uint16), L.dev_ptr(mask, torch.uint8, True), sc, records_before, L.dev_ptr(ints), L.dev_ptr(floats),
          L.dev_ptr(ws), L.IRS_TRUTH_UPDATE_WS_BYTES)
    return ints, floats


def _doubles(values):
    values = [float(v) for v in values]
    return (C.c_double * max(len(values), 1))(*values), len(values)


def truth_calibrate(mean, comoment, below, truth, n, scale, d2_edges, levels, rank_bins, var_edges, std_floor=1e-3, mask=None,
                    workspace=None):
    """A displacement covariance state against the truth.  mean (3,D,H,W), comoment (6,D,H,W: xx, yy, zz, xy, xz, yz) float32
    after n >= 2 records (ops.displacement_covariance_update); below (3,D,H,W) uint16 of truth_update after the same records;
    truth (3,D,H,W) float32; scale: three finite floats > 0; d2_edges: the B - 1 strictly increasing edges of the B PIT bins of
    d^2; levels: 1..8 thresholds of d^2; rank_bins: B_r; var_edges: the R - 1 strictly increasing edges of the R reliability bins
    of the predicted total variance; std_floor: f > 0; mask (D,H,W) bool / uint8 or None.  -> dict, everything on the device:
    'error', 'mahalanobis' (D,H,W) float32 (independent of the mask); 'pit_hist' (B,), 'coverage' (L,), 'rank_hist' (3,B_r) int64
    (views of one array); 'rel_ints' (R,1) int64, 'rel_floats' (R,2) float64 {sum v, sum |Delta|^2}; 'isummary' (3,) int64
    SUMMARY_INT_COLUMNS, 'fsummary' (9,) float64 SUMMARY_FLOAT_COLUMNS: include/irsgmcmc.h gives the definitions
    (irs_truth_calibrate).  No host synchronisation."""
    if mean.dim() != 4:
        raise L.IrsError(f'mean must have shape (3,D,H,W), got {tuple(mean.shape)}')
    D, H, W = mean.shape[1:]
    _check_state(('mean', mean, (3, D, H, W), torch.float32), ('comoment', comoment, (6, D, H, W), torch.float32))
    _truth_state(truth, below, (D, H, W))
    if isinstance(n, bool) or int(n) != n:
        raise L.IrsError(f'n must be an integer number of records, got {n!r}')
    mask = _volume_mask(mask, D, H, W)
    sc = _three_positive('scale', scale)
    if isinstance(std_floor, bool) or not isinstance(std_floor, numbers.Real):
        raise L.IrsError(f'std_floor must be a finite number > 0, got {std_floor!r}')
    if isinstance(rank_bins, bool) or int(rank_bins) != rank_bins:
        raise L.IrsError(f'rank_bins must be an integer, got {rank_bins!r}')
    (e2, ne), (lv, nl), (ve, nv) = _doubles(d2_edges), _doubles(levels), _doubles(var_edges)
    B, Br, R = ne + 1, int(rank_bins), nv + 1
    dev = mean.device
    # (the counts are sized for the caps: a refused call must not depend on a size it refuses)
    counts = torch.empty(max(B, 1) + max(nl, 1) + 3 * min(max(Br, 1), L.IRS_TRUTH_MAX_BINS), device=dev, dtype=torch.int64)
    rel_ints = torch.empty((max(R, 1), L.IRS_TRUTH_RELIABILITY_INTS), device=dev, dtype=torch.int64)
    rel_floats = torch.empty((max(R, 1), L.IRS_TRUTH_RELIABILITY_FLOATS), device=dev, dtype=torch.float64)
    isummary = torch.empty(L.IRS_TRUTH_SUMMARY_INTS, device=dev, dtype=torch.int64)
    fsummary = torch.empty(L.IRS_TRUTH_SUMMARY_FLOATS, device=dev, dtype=torch.float64)
    error, mahalanobis = (torch.empty((D, H, W), device=dev, dtype=torch.float32) for _ in range(2))
    ws = (workspace or TruthWorkspace(dev)).calibrate
    _call('irs_truth_calibrate', L.dev_ptr(mean, torch.float32), L.dev_ptr(comoment, torch.float32), L.dev_ptr(below, torch.uint16),
          L.dev_ptr(truth, torch.float32), D, H, W, int(n), sc, float(std_floor), L.dev_ptr(mask, torch.uint8, True), e2, B, lv, nl,
          Br, ve, R, L.dev_ptr(error), L.dev_ptr(mahalanobis), L.dev_ptr(counts), L.dev_ptr(rel_ints), L.dev_ptr(rel_floats),
          L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws), L.IRS_TRUTH_CALIBRATE_WS_BYTES)
    return {'error': error, 'mahalanobis': mahalanobis, 'counts': counts, 'pit_hist': counts[:B], 'coverage': counts[B:B + nl],
            'rank_hist': counts[B + nl:B + nl + 3 * Br].view(3, Br), 'rel_ints': rel_ints, 'rel_floats': rel_floats,
            'isummary': isummary, 'fsummary': fsummary}


# ---------------------------------------------------------------- thresholds and the host summary (float64)
def _levels(levels, what):
    try:
        out = [float(v) for v in levels]
    except (TypeError, ValueError):
        raise ValueError(f'{what} must be a list of probabilities, got {levels!r}') from None
    if not 1 <= len(out) <= L.IRS_TRUTH_MAX_LEVELS:
        raise ValueError(f'{what} must hold 1..{L.IRS_TRUTH_MAX_LEVELS} levels, got {len(out)}')
    if any(isinstance(v, bool) for v in levels) or not all(0.0 < v < 1.0 for v in out) or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f'{what} must be strictly increasing in (0,1), got {list(levels)}')
    return tuple(out)


def d2_quantile(p, n, reference='hotelling'):
    """the p-quantile(s) of d^2 = (mean - t)^T S^-1 (mean - t) for a truth drawn from the law of the n records: "hotelling":
    (1 + 1/n) 3 (n - 1) / (n - 3) F^-1_{3, n-3}(p), n >= 4; "chi2": the quantile of chi^2_3.  scipy.stats on the host."""
    from scipy import stats
    p = np.asarray(p, dtype=np.float64)
    if reference == 'chi2':
        return stats.chi2.ppf(p, 3)
    if reference != 'hotelling':
        raise ValueError(f'reference must be one of {list(REFERENCES)}, got {reference!r}')
    n = int(n)
    if n < 4:
        raise ValueError(f'the Hotelling reference needs n >= 4 records, got {n}')
    return (1.0 + 1.0 / n) * 3.0 * (n - 1.0) / (n - 3.0) * stats.f.ppf(p, 3, n - 3)


def expected_scale(n, reference='hotelling'):
    """sqrt(E d^2 / 3) of a calibrated posterior: "hotelling": sqrt((1 + 1/n) (n - 1) / (n - 5)) (NaN for n <= 5); "chi2": 1"""
    if reference == 'chi2':
        return 1.0
    n = int(n)
    return math.sqrt((1.0 + 1.0 / n) * (n - 1.0) / (n - 5.0)) if n > 5 else math.nan


def calibration_thresholds(n, levels=(0.5, 0.9, 0.95), pit_bins=20, reference='hotelling'):
    """-> (d2_edges: the pit_bins - 1 quantiles of d^2 at b / pit_bins, level thresholds: its quantiles at `levels`), float64"""
    B = int(pit_bins)
    if not 1 <= B <= L.IRS_TRUTH_MAX_BINS:
        raise ValueError(f'pit_bins must be in 1..{L.IRS_TRUTH_MAX_BINS}, got {pit_bins!r}')
    return (d2_quantile(np.arange(1, B) / B, n, reference), d2_quantile(np.asarray(_levels(levels, 'levels')), n, reference))


def default_var_edges(reliability_bins, std_range=RELIABILITY_STD_RANGE):
    """the R - 1 edges of the reliability bins of the predicted total variance: squares of R - 1 stds spaced geometrically over
    std_range (one edge, at the geometric middle, for R = 2; none for R = 1)"""
    R = int(reliability_bins)
    if not 1 <= R <= L.IRS_TRUTH_MAX_RELIABILITY_BINS:
        raise ValueError(f'reliability_bins must be in 1..{L.IRS_TRUTH_MAX_RELIABILITY_BINS}, got {reliability_bins!r}')
    lo, hi = (float(s) for s in std_range)
    if R == 1:
        return np.zeros(0)
    if R == 2:
        return np.asarray([lo * hi])
    return np.geomspace(lo, hi, R - 1) ** 2


def rank_expected_fractions(n, rank_bins):
    """the exact probability of every rank bin for a calibrated posterior: the rank `below` of the truth among n records is
    uniform on 0 .. n, and bin b holds the ranks r with floor(r B_r / (n + 1)) == b -- unequal shares unless (n + 1) % B_r == 0"""
    n, Br = int(n), int(rank_bins)
    return np.bincount(np.arange(n + 1) * Br // (n + 1), minlength=Br).astype(np.float64) / (n + 1)


def _chi2(observed, expected):
    """sum (o - e)^2 / e over the bins with e > 0 (NaN when nothing was observed)"""
    observed, expected = np.asarray(observed, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    if not observed.sum() > 0:
        return math.nan
    keep = expected > 0
    return float(np.sum((observed[keep] - expected[keep]) ** 2 / expected[keep]))


def error_stats(ints, floats):
    """(voxels, non_finite), (sum r, sum r^2, max r) of truth_update or the first columns of truth_calibrate -> {'mean', 'rmse',
    'max'} over the finite masked voxels (NaN when there is none)"""
    voxels, nonfinite = int(ints[0]), int(ints[1])
    finite = voxels - nonfinite
    if finite <= 0:
        return {'mean': math.nan, 'rmse': math.nan, 'max': math.nan}
    return {'mean': float(floats[0]) / finite, 'rmse': math.sqrt(float(floats[1]) / finite), 'max': float(floats[2])}


def calibration_summary(isummary, fsummary, pit_hist, coverage, rank_hist, rel_ints, rel_floats, n, levels, reference='hotelling',
                        var_edges=None, initial=None, floor=None):
    """The derived numbers of truth_calibrate's reduced outputs (host ints / floats or arrays), n records, on the host in float64:
    'records', 'reference', 'voxels', 'nonfinite_voxels', 'raised_voxels'; 'mean', 'rmse', 'max' of the error of the posterior mean
    and 'initial_{mean,rmse,max}' of the identity's (`initial`: the dict of error_stats of a zero displacement; NaN when None);
    'coverage': {level: {'nominal', 'observed', 'count'}}; 'pit_hist', 'pit_chi2' and 'pit_ks' against uniform (the largest
    distance of the cumulative histogram from b / B at the bin edges); 'rank_hist' (3 lists), 'rank_expected' (the exact expected
    counts, rank_expected_fractions) and 'rank_chi2_{x,y,z}' against them; 'z_rms_{x,y,z}' = sqrt(mean Delta_c^2 / A_cc);
    'd2_mean', 'd2_max'; 'scale_factor_raw' = sqrt(sum d^2 / 3 V), 'scale_factor_expected' (expected_scale) and 'scale_factor',
    their ratio: the single number the posterior std would have to be multiplied by; 'std_total' = sqrt(mean v); 'reliability':
    rows {'var_lo', 'var_hi', 'count', 'std_predicted' = sqrt(mean v), 'rmse_observed' = sqrt(mean |Delta|^2)} and 'ence', the mean
    over the non-empty bins of |std_predicted - rmse_observed| / std_predicted; 'floor_mean', 'floor_max' (`floor`: known_pair's
    info; NaN when None) and 'below_floor': whether the mean error lies below the truth's own mean error floor, where it means
    nothing.  Float entries are NaN for an empty mask or when no masked voxel is finite."""
    n = int(n)
    voxels, nonfinite, raised = (int(x) for x in np.asarray(isummary).reshape(-1))
    f = [float(x) for x in np.asarray(fsummary, dtype=np.float64).reshape(-1)]
    finite = voxels - nonfinite
    nan = math.nan
    levels = _levels(levels, 'levels')
    pit = np.asarray(pit_hist, dtype=np.int64).reshape(-1)
    cov = np.asarray(coverage, dtype=np.int64).reshape(-1)
    rank = np.asarray(rank_hist, dtype=np.int64).reshape(3, -1)
    if len(cov) != len(levels):
        raise ValueError(f'calibration_summary: {len(cov)} coverage counts for {len(levels)} levels')
    out = {'records': n, 'reference': reference, 'voxels': voxels, 'nonfinite_voxels': nonfinite, 'raised_voxels': raised}
    out.update(error_stats((voxels, nonfinite), f[:3]))
    init = initial or {}
    out.update({f'initial_{k}': float(init.get(k, nan)) for k in ('mean', 'rmse', 'max')})
    out['coverage'] = {coverage_key(lv): {'nominal': lv, 'observed': int(c) / finite if finite else nan, 'count': int(c)}
                       for lv, c in zip(levels, cov)}
    B = len(pit)
    out['pit_hist'] = pit.tolist()
    out['pit_chi2'] = _chi2(pit, np.full(B, finite / B)) if finite else nan
    out['pit_ks'] = float(np.max(np.abs(np.cumsum(pit) / finite - np.arange(1, B + 1) / B))) if finite else nan
    fractions = rank_expected_fractions(n, rank.shape[1])
    out['rank_hist'] = rank.tolist()
    out['rank_expected'] = (fractions * finite).tolist()
    for c, axis in enumerate('xyz'):
        out[f'rank_chi2_{axis}'] = _chi2(rank[c], fractions * finite) if finite else nan
        out[f'z_rms_{axis}'] = math.sqrt(f[6 + c] / finite) if finite and f[6 + c] >= 0 else nan
    out['d2_mean'], out['d2_max'] = (f[3] / finite, f[4]) if finite else (nan, nan)
    out['scale_factor_raw'] = math.sqrt(f[3] / (3.0 * finite)) if finite and f[3] >= 0 else nan
    out['scale_factor_expected'] = expected_scale(n, reference)
    out['scale_factor'] = out['scale_factor_raw'] / out['scale_factor_expected']
    out['std_total'] = math.sqrt(f[5] / finite) if finite and f[5] >= 0 else nan
    counts = np.asarray(rel_ints, dtype=np.int64).reshape(-1)
    sums = np.asarray(rel_floats, dtype=np.float64).reshape(-1, 2)
    R = len(counts)
    edges = default_var_edges(R) if var_edges is None else np.asarray(var_edges, dtype=np.float64).reshape(-1)
    lo, hi = np.concatenate([[-np.inf], edges]), np.concatenate([edges, [np.inf]])
    rows, terms = [], []
    for b in range(R):
        k = int(counts[b])
        row = {'var_lo': float(lo[b]), 'var_hi': float(hi[b]), 'count': k, 'std_predicted': nan, 'rmse_observed': nan}
        if k > 0 and sums[b, 0] > 0:
            row['std_predicted'], row['rmse_observed'] = math.sqrt(sums[b, 0] / k), math.sqrt(max(sums[b, 1], 0.0) / k)
            terms.append(abs(row['std_predicted'] - row['rmse_observed']) / row['std_predicted'])
        rows.append(row)
    out['reliability'] = rows
    out['ence'] = float(np.mean(terms)) if terms else nan
    fl = floor or {}
    out['floor_mean'], out['floor_max'] = float(fl.get('floor_mean', nan)), float(fl.get('floor_max', nan))
    out['below_floor'] = bool(out['mean'] < out['floor_mean'])
    return out


def coverage_key(level):
    """0.9 -> '90', 0.95 -> '95', 0.995 -> '99.5': the XX of the coverage_XX metrics"""
    return f'{100 * float(level):g}'


# ---------------------------------------------------------------- the trainer's option, metric names and files
def _int(opt, key, lo, hi, what):
    v = opt[key]
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= int(v) <= hi:
        raise ValueError(f'{what}.{key} must be an integer in {lo}..{hi}, got {v!r}')
    return int(v)


def _real(opt, key, ok, words, what):
    v = opt[key]
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or not ok(v):
        raise ValueError(f'{what}.{key} must be {words}, got {v!r}')
    return float(v)


def truth_options(cfg_trainer):
    """`trainer.truth` -> None when off (absent / false / null), else the dict of OPTION_KEYS with the defaults filled in:
    {"source": "simulate" | "file", "seed", "amplitude", "modes", "max_wavenumber", "noise" (simulate), "path", "unit": "voxels" |
    "mm" (file), "period" (default log_period_MCMC), "levels": [0.5, 0.9, 0.95], "pit_bins": 20, "rank_bins": 16,
    "reliability_bins": 16, "std_floor": 1e-3, "reference": "hotelling" | "chi2", "save": true}.  Refuses, with the offending
    value: anything but a dict; unknown keys; a missing or unknown source; a key of the other source; bad values; what
    diagnostics._record_options refuses (and more than 65535 records, what a uint16 rank count holds); MCMC: false; fewer records
    than the reference needs (6 for "hotelling", whose expected factor has n - 5 in it, 2 for "chi2"); trainer.affine_init (the
    truth would have to be composed with the pre-alignment); and with "simulate", the options that read other files on the
    original moving image's grid: native_resolution, native_posterior, landmarks and image_posterior volumes."""
    from .diagnostics import _record_options
    what = 'trainer.truth'
    raw = cfg_trainer.get('truth', False)
    if raw is not None and raw is not False and not isinstance(raw, dict):
        raise ValueError(f'{what} must be false or {{"source": "simulate" | "file", ...}}, got {raw!r}')

    def own_keys(opt):
        if opt.get('source') not in SOURCES:
            raise ValueError(f'{what}.source must be one of {list(SOURCES)}, got {opt.get("source")!r}')
        source = opt['source']
        foreign = [k for k in (FILE_KEYS if source == 'simulate' else SIMULATE_KEYS) if k in opt]
        if foreign:
            raise ValueError(f'{what}: keys {foreign} do not go with "source": {source!r}')
        o = {**OPTION_DEFAULTS, **{k: v for k, v in opt.items() if k != 'period'}}
        out = {'source': source}
        seed = o['seed']
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or seed < 0:
            raise ValueError(f'{what}.seed must be an integer >= 0, got {seed!r}')
        out['seed'] = int(seed)
        out['amplitude'] = _real(o, 'amplitude', lambda v: v >= 0, 'a finite number >= 0 (voxels)', what)
        out['modes'] = _int(o, 'modes', 1, 64, what)
        out['max_wavenumber'] = _int(o, 'max_wavenumber', 1, 16, what)
        out['noise'] = _real(o, 'noise', lambda v: v >= 0, 'a finite number >= 0', what)
        if source == 'file' and (not isinstance(o['path'], str) or not o['path']):
            raise ValueError(f'{what}.path must name the truth file, got {o["path"]!r}')
        out['path'] = o['path']
        if o['unit'] not in UNITS:
            raise ValueError(f'{what}.unit must be one of {list(UNITS)}, got {o["unit"]!r}')
        out['unit'] = o['unit']
        out['levels'] = _levels(o['levels'], f'{what}.levels')
        out['pit_bins'] = _int(o, 'pit_bins', 2, L.IRS_TRUTH_MAX_BINS, what)
        out['rank_bins'] = _int(o, 'rank_bins', 2, L.IRS_TRUTH_MAX_BINS, what)
        out['reliability_bins'] = _int(o, 'reliability_bins', 1, L.IRS_TRUTH_MAX_RELIABILITY_BINS, what)
        out['std_floor'] = _real(o, 'std_floor', lambda v: v > 0 and v * v > 0, 'a finite number > 0', what)
        if o['reference'] not in REFERENCES:
            raise ValueError(f'{what}.reference must be one of {list(REFERENCES)}, got {o["reference"]!r}')
        out['reference'] = o['reference']
        if not isinstance(o['save'], bool):
            raise ValueError(f'{what}.save must be true or false, got {o["save"]!r}')
        out['save'] = o['save']
        return out

    out = _record_options(cfg_trainer, 'truth', OPTION_KEYS, '{"source": "simulate" | "file", ...}', L.IRS_TRUTH_MAX_RECORDS,
                          'a uint16 rank count holds at most {}', own_keys)
    if out is None:
        return None
    if not cfg_trainer.get('MCMC', True):
        raise ValueError(f'{what} needs the MCMC stage: MCMC is false')
    records = (int(cfg_trainer['no_samples_MCMC']) // out['period']) * int(cfg_trainer.get('no_chains', 1))
    if records < MIN_RECORDS[out['reference']]:
        raise ValueError(f'{what}: {records} records, at least {MIN_RECORDS[out["reference"]]} needed with "reference": '
                         f'{out["reference"]!r}')
    if cfg_trainer.get('affine_init'):
        raise ValueError(f'{what} cannot be combined with trainer.affine_init: the truth would have to be composed with the '
                         f'pre-alignment')
    if out['source'] == 'simulate':
        for key in ('native_resolution', 'native_posterior', 'landmarks'):
            if cfg_trainer.get(key):
                raise ValueError(f'{what} with "source": "simulate" cannot be combined with trainer.{key}, which reads files on the '
                                 f'original moving image\'s grid: the moving triple is replaced')
        image = cfg_trainer.get('image_posterior')
        if isinstance(image, dict) and image.get('volumes'):
            raise ValueError(f'{what} with "source": "simulate" cannot be combined with trainer.image_posterior.volumes '
                             f'{image["volumes"]!r}: volumes on the original moving image\'s grid')
    return out


METRIC_KEYS = ('rmse', 'mean', 'max', 'scale_factor', 'ence', 'pit_chi2', 'pit_ks', 'rank_chi2_x', 'rank_chi2_y', 'rank_chi2_z',
               'z_rms_x', 'z_rms_y', 'z_rms_z')
INITIAL_METRICS = ('rmse', 'mean', 'max')


def truth_metric_names(options):
    """truth/initial/{rmse,mean,max} of step 0, then MCMC/truth/{METRIC_KEYS} and MCMC/truth/coverage_XX per level"""
    return ([f'truth/initial/{k}' for k in INITIAL_METRICS] + [f'MCMC/truth/{k}' for k in METRIC_KEYS] +
            [f'MCMC/truth/coverage_{coverage_key(lv)}' for lv in options['levels']])


def calibration_csv(summary):
    """(header, rows) of samples/MCMC_truth_calibration.csv: one long table, `table` naming the part -- 'pit' (bin, count,
    expected), 'rank_x' / 'rank_y' / 'rank_z' (bin, count, expected), 'reliability' (bin, count, and in the two value columns the
    predicted std and the observed RMSE; lo / hi: the bin's variance range), 'coverage' (bin = the level's XX, count, expected =
    nominal * voxels; value_a = observed, value_b = nominal).  Floats by repr: they read back exactly."""
    header = ['table', 'bin', 'count', 'expected', 'lo', 'hi', 'value_a', 'value_b']
    finite = summary['voxels'] - summary['nonfinite_voxels']
    rows = []
    B = len(summary['pit_hist'])
    for b, k in enumerate(summary['pit_hist']):
        rows.append(['pit', str(b), str(int(k)), repr(finite / B), repr(b / B), repr((b + 1) / B), repr(math.nan), repr(math.nan)])
    for c, axis in enumerate('xyz'):
        for b, k in enumerate(summary['rank_hist'][c]):
            rows.append([f'rank_{axis}', str(b), str(int(k)), repr(float(summary['rank_expected'][b])), repr(math.nan), repr(math.nan),
                         repr(math.nan), repr(math.nan)])
    for b, row in enumerate(summary['reliability']):
        rows.append(['reliability', str(b), str(row['count']), repr(math.nan), repr(row['var_lo']), repr(row['var_hi']),
                     repr(row['std_predicted']), repr(row['rmse_observed'])])
    for key, row in summary['coverage'].items():
        rows.append(['coverage', key, str(row['count']), repr(row['nominal'] * finite), repr(math.nan), repr(math.nan),
                     repr(row['observed']), repr(row['nominal'])])
    return header, rows


def series_csv(ints, floats, steps, chains):
    """(header, rows) of samples/MCMC_truth_series.csv: per record SERIES_COLUMNS -- the record's number, the transition it was
    taken at, its chain, the mean, RMS and max error of that sample over the mask, the masked voxels and the non-finite ones"""
    ints, floats = np.asarray(ints, dtype=np.int64), np.asarray(floats, dtype=np.float64)
    rows = []
    for r in range(len(ints)):
        e = error_stats(ints[r], floats[r])
        rows.append([str(r), str(int(steps[r // chains])), str(r % chains), repr(e['mean']), repr(e['rmse']), repr(e['max']),
                     str(int(ints[r, 0])), str(int(ints[r, 1]))])
    return list(SERIES_COLUMNS), rows
