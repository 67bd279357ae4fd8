"""Posterior comparison: does the variational posterior describe the same registration uncertainty as the SG-MCMC chains, and
where do they differ?

The reference writes the displacement mean / std of the VI test samples and of the MCMC samples side by side and compares
nothing.  Here each side is a `diagnostics.DisplacementCovariance` state -- the Welford mean and co-moments of the displacement
per voxel -- and `posterior_compare` gives, per voxel, the distances between the two 3-D Gaussians those states describe: the
mean shift, the log ratio of the total spreads, the Bures distance of the covariances (with the shift, the 2-Wasserstein
distance) and the Jeffreys divergence; one HIP pass (include/irsgmcmc.h: irs_posterior_compare).  `comparison_summary` turns
its reduced columns into the numbers that are logged.

The operator wrapper lives here and not in ops.py; it uses its private helpers.
"""
import math
import numbers

import torch

from . import _lib as L
from .ops import _call, _check_state, _summary_buffers, _three_positive, _volume_mask

COMPARISON_PLANES = ('shift', 'log_std_ratio', 'bures', 'jeffreys')


def _records(name, n):
    if isinstance(n, bool) or int(n) != n or int(n) < 2:
        raise L.IrsError(f'{name} must be an integer number of records >= 2, got {n!r}')
    return int(n)


def posterior_compare(mean_a, comoment_a, n_a, mean_b, comoment_b, n_b, scale, std_floor=1e-3, mask=None):
    """The distances between the Gaussians of two displacement covariance states A and B.  mean_x (3,D,H,W) and comoment_x
    (6,D,H,W: xx, yy, zz, xy, xz, yz) float32 after n_x >= 2 records (ops.displacement_covariance_update); scale: three
    positive floats, one per channel; std_floor: f > 0; mask (D,H,W) bool / uint8 or None.  -> (shift, log_std_ratio, bures,
    jeffreys, all (D,H,W) float32, isummary (4,) int64, fsummary (13,) float64), all on the device: include/irsgmcmc.h gives
    the definitions and the columns.  log_std_ratio < 0: A is the narrower.  No host synchronisation."""
    if mean_a.dim() != 4:
        raise L.IrsError(f'mean_a must have shape (3,D,H,W), got {tuple(mean_a.shape)}')
    D, H, W = mean_a.shape[1:]
    _check_state(('mean_a', mean_a, (3, D, H, W), torch.float32), ('comoment_a', comoment_a, (6, D, H, W), torch.float32),
                 ('mean_b', mean_b, (3, D, H, W), torch.float32), ('comoment_b', comoment_b, (6, D, H, W), torch.float32))
    n_a, n_b = _records('n_a', n_a), _records('n_b', n_b)
    mask = _volume_mask(mask, D, H, W)
    scale = _three_positive('scale', scale)
    if isinstance(std_floor, bool) or not isinstance(std_floor, numbers.Real) or not math.isfinite(std_floor) or not std_floor > 0:
        raise L.IrsError(f'std_floor must be a finite number > 0, got {std_floor!r}')
    dev = mean_a.device
    ws, isummary, fsummary = _summary_buffers(L.IRS_COMPARE_WS_BYTES, L.IRS_COMPARE_SUMMARY_INTS, L.IRS_COMPARE_SUMMARY_FLOATS, dev)
    planes = [torch.empty((D, H, W), device=dev, dtype=torch.float32) for _ in COMPARISON_PLANES]
    _call('irs_posterior_compare', L.dev_ptr(mean_a, torch.float32), L.dev_ptr(comoment_a, torch.float32), n_a,
          L.dev_ptr(mean_b, torch.float32), L.dev_ptr(comoment_b, torch.float32), n_b, D, H, W, scale, float(std_floor),
          L.dev_ptr(mask, torch.uint8, True), *(L.dev_ptr(p) for p in planes), L.dev_ptr(isummary), L.dev_ptr(fsummary),
          L.dev_ptr(ws), L.IRS_COMPARE_WS_BYTES)
    return (*planes, isummary, fsummary)


def comparison_summary(isummary, fsummary, n_a, n_b):
    """the summary of DESIGN.md section 6 from posterior_compare's reduced columns (host ints / floats), A the VI side of n_a
    records and B the MCMC side of n_b: isummary {voxels, voxels with a non-finite state, voxels with a floored eigenvalue,
    voxels with log_std_ratio < 0}, fsummary {sum / max shift, sum / min / max log_std_ratio, sum / max bures, sum / max w2, sum
    / max jeffreys, sum tr S_A, sum tr S_B} over the finite masked voxels.  'std_ratio' = exp of the mean log ratio: the
    geometric mean of the VI spread over the MCMC spread; 'frac_vi_narrower': the share of voxels with log_std_ratio < 0;
    'std_total_*' = sqrt of the mean trace.  The float entries are NaN for an empty mask or when no masked voxel is finite."""
    voxels, nonfinite, floored, narrower = (int(x) for x in isummary)
    (sh_sum, sh_max, lr_sum, lr_min, lr_max, bu_sum, bu_max, w2_sum, w2_max, je_sum, je_max, tra_sum, trb_sum) = (float(x) for x in fsummary)
    finite = voxels - nonfinite
    nan = float('nan')
    mean = lambda total: total / finite if finite else nan
    extreme = lambda value: value if finite else nan
    return {'records_vi': int(n_a), 'records_mcmc': int(n_b), 'voxels': voxels, 'nonfinite_voxels': nonfinite, 'floored_voxels': floored,
            'shift_mean': mean(sh_sum), 'shift_max': extreme(sh_max),
            'log_std_ratio_mean': mean(lr_sum), 'log_std_ratio_min': extreme(lr_min), 'log_std_ratio_max': extreme(lr_max),
            'std_ratio': math.exp(lr_sum / finite) if finite else nan, 'frac_vi_narrower': mean(float(narrower)),
            'bures_mean': mean(bu_sum), 'bures_max': extreme(bu_max), 'w2_mean': mean(w2_sum), 'w2_max': extreme(w2_max),
            'jeffreys_mean': mean(je_sum), 'jeffreys_max': extreme(je_max),
            'std_total_vi': math.sqrt(max(tra_sum / finite, 0.0)) if finite else nan,
            'std_total_mcmc': math.sqrt(max(trb_sum / finite, 0.0)) if finite else nan}
