"""Residual model check: does the likelihood describe the residuals it is applied to, and where does it not?

The data term models the residual z as a zero-mean Gaussian mixture (`model.loss.GMM`; `SSD` is one Gaussian).  The reference
draws the histogram of the masked residuals under the mixture's density (log_hist_res, logger/visualization.py:64-86); this
module gives the same check as numbers:

 - `residual_histogram`: per chain the histogram, the counts and the moment sums of z, one HIP pass over the volumes
   (include/irsgmcmc.h: irs_residual_histogram), accumulated exactly over calls;
 - `residual_fit`: those against the mixture -- the divergences of the binned distributions and the moment ratios -- on the
   host in float64 (at most 512 numbers per chain: no hot path);
 - `residual_nll_update` / `residual_nll_finalize`: the per-voxel posterior mean of -log p(z) and its masked summary.

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .ops import _call, _check_state, _dims5, _shared_mask, _summary_buffers, _volume_mask

RESIDUAL_COUNTS = ('n', 'n_nonfinite', 'n_clipped')
RESIDUAL_SUMS = ('sum_z', 'sum_z2', 'sum_z4', 'max_abs_z')
FIT_KEYS = ('kl', 'tv', 'ks', 'chi2', 'tail', 'tail_model', 'mean', 'std', 'std_model', 'kurtosis', 'kurtosis_model', 'n')


def residual_histogram(residuals, mask, half_range, bins, hist=None, counts=None, sums=None, records_before=0):
    """The histogram and the moments of the residuals: residuals (C,1,D,H,W) float32; mask (1,1,D,H,W) bool / uint8 shared by the
    chains, or None; bins in 2 .. 512 equal bins over [-half_range, half_range], half_range finite and > 0 (as float32).  ->
    {'hist': (C,bins) int64, 'counts': (C,3) int64 RESIDUAL_COUNTS, 'sums': (C,4) float64 RESIDUAL_SUMS} on the device.  The
    three tensors accumulate over calls: pass them back in with `records_before` > 0 and this call's integers and sums are
    added (the maximum merged); `records_before` = 0 overwrites them (or allocates them).  No host synchronisation
    (include/irsgmcmc.h: irs_residual_histogram)."""
    Cn, D, H, W = _dims5(residuals, 1)
    mask = _shared_mask(mask, D, H, W)
    if isinstance(bins, bool) or not isinstance(bins, int):
        raise L.IrsError(f'bins must be an integer, got {bins!r}')
    records_before = int(records_before)
    dev = residuals.device
    state = {'hist': hist, 'counts': counts, 'sums': sums}
    missing = [name for name, t in state.items() if t is None]
    if missing and records_before > 0:
        raise L.IrsError(f'records_before = {records_before} needs the state of the earlier calls; {missing} not given')
    shapes = {'hist': ((Cn, bins), torch.int64), 'counts': ((Cn, 3), torch.int64), 'sums': ((Cn, 4), torch.float64)}
    for name in missing:
        state[name] = torch.empty(shapes[name][0], device=dev, dtype=shapes[name][1])
    _check_state(*((name, state[name], *shapes[name]) for name in state))
    ws = torch.empty(L.IRS_RESIDUAL_WS_BYTES, device=dev, dtype=torch.uint8)
    _call('irs_residual_histogram', L.dev_ptr(residuals, torch.float32), Cn, L.dev_ptr(mask, torch.uint8, True), D, H, W,
          float(half_range), bins, L.dev_ptr(state['hist']), L.dev_ptr(state['counts']), L.dev_ptr(state['sums']), records_before,
          L.dev_ptr(ws), L.IRS_RESIDUAL_WS_BYTES)
    return state


def _doubles(name, values, K=None):
    values = [float(v) for v in (values.tolist() if hasattr(values, 'tolist') else values)]
    if K is not None and len(values) != K:
        raise L.IrsError(f'{name} must hold {K} numbers, got {len(values)}')
    return values


def residual_nll_update(residuals, log_weight, inv_std, mean, count, records_before):
    """Fold one recorded step of residuals into the per-voxel posterior mean of the negative log-likelihood under a mixture:
    residuals (C,1,D,H,W) float32; log_weight[k] = ln pi_k - ln sigma_k - 1/2 ln 2 pi and inv_std[k] = 1 / sigma_k, K in 1 .. 8
    host numbers each (mixture_terms); mean (D,H,W) float32 and count (D,H,W) int32: the streaming mean and the number of the
    finite residuals, folded in chain order after `records_before` records (0 overwrites the state).  No host synchronisation
    (include/irsgmcmc.h: irs_residual_nll_update)."""
    Cn, D, H, W = _dims5(residuals, 1)
    _check_state(('mean', mean, (D, H, W), torch.float32), ('count', count, (D, H, W), torch.int32))
    log_weight = _doubles('log_weight', log_weight)
    inv_std = _doubles('inv_std', inv_std, len(log_weight))
    K = len(log_weight)
    array = C.c_double * max(K, 1)
    _call('irs_residual_nll_update', L.dev_ptr(residuals, torch.float32), Cn, D, H, W, array(*log_weight), array(*inv_std), K,
          L.dev_ptr(mean), L.dev_ptr(count), int(records_before))


def residual_nll_finalize(mean, count, mask=None):
    """The masked summary of the NLL state.  mean (D,H,W) float32, count (D,H,W) int32; mask (D,H,W) bool / uint8 or None.  ->
    (isummary (2,) int64 {voxels, voxels with count == 0}, fsummary (2,) float64 {sum of mean, max of mean} over the voxels
    with count > 0), on the device.  No host synchronisation."""
    if mean.dim() != 3:
        raise L.IrsError(f'mean must have shape (D,H,W), got {tuple(mean.shape)}')
    D, H, W = mean.shape
    _check_state(('mean', mean, (D, H, W), torch.float32), ('count', count, (D, H, W), torch.int32))
    mask = _volume_mask(mask, D, H, W)
    ws, isummary, fsummary = _summary_buffers(L.IRS_RESIDUAL_MAP_WS_BYTES, L.IRS_RESIDUAL_MAP_SUMMARY_INTS,
                                              L.IRS_RESIDUAL_MAP_SUMMARY_FLOATS, mean.device)
    _call('irs_residual_nll_finalize', L.dev_ptr(mean), L.dev_ptr(count), L.dev_ptr(mask, torch.uint8, True), D, H, W,
          L.dev_ptr(isummary), L.dev_ptr(fsummary), L.dev_ptr(ws), L.IRS_RESIDUAL_MAP_WS_BYTES)
    return isummary, fsummary


_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def mixture_terms(data_loss):
    """the likelihood of a data loss as a zero-mean mixture -> (std, proportions, log_weight, inv_std), four lists of K
    float64: sigma_k, pi_k, ln pi_k - ln sigma_k - 1/2 ln 2 pi and 1 / sigma_k.  A GMM (after the trainer's sync_parameters)
    gives its own log_proportions -- log_softmax(logits + 1e-2) -- and log_std; an SSD one component with sigma and pi = 1."""
    if hasattr(data_loss, 'log_proportions') and hasattr(data_loss, 'log_std'):
        with torch.no_grad():
            log_pi = data_loss.log_proportions.detach().to('cpu', torch.float64).tolist()
            log_std = data_loss.log_std.detach().to('cpu', torch.float64).tolist()
    elif hasattr(data_loss, 'sigma'):
        sigma = float(data_loss.sigma)
        if not (math.isfinite(sigma) and sigma > 0):
            raise ValueError(f'mixture_terms: sigma = {sigma}, a finite value > 0 needed')
        log_pi, log_std = [0.0], [math.log(sigma)]
    else:
        raise TypeError(f'mixture_terms: {type(data_loss).__name__} is neither a Gaussian mixture nor an SSD')
    return ([math.exp(s) for s in log_std], [math.exp(p) for p in log_pi],
            [p - s - _HALF_LOG_2PI for p, s in zip(log_pi, log_std)], [math.exp(-s) for s in log_std])


def mixture_cdf(x, std, proportions):
    """F(x) = sum_k pi_k 1/2 erfc(-x / (sigma_k sqrt 2))"""
    return sum(p * 0.5 * math.erfc(-x / (s * math.sqrt(2.0))) for s, p in zip(std, proportions))


def bin_edges(half_range, bins):
    """the bins + 1 edges e_b = -h + 2 h b / bins"""
    h = float(half_range)
    return [-h + 2.0 * h * b / bins for b in range(bins + 1)]


def model_probabilities(half_range, bins, std, proportions):
    """p_b of the bins under the mixture -> (p (bins,) float64, F at the bins + 1 edges).  p_b = F(e_b+1) - F(e_b); the end
    bins take the tails: p_0 = F(e_1) and p_(bins-1) = 1/2 sum pi_k erfc(e_(bins-1) / (sigma_k sqrt 2))."""
    edges = bin_edges(half_range, bins)
    F = [mixture_cdf(e, std, proportions) for e in edges]
    p = np.array([F[b + 1] - F[b] for b in range(bins)], dtype=np.float64)
    p[0] = F[1]
    p[bins - 1] = 0.5 * sum(pk * math.erfc(edges[bins - 1] / (s * math.sqrt(2.0))) for s, pk in zip(std, proportions))
    return p, F


def _fit_one(hist, counts, sums, half_range, std, proportions):
    bins = len(hist)
    n = int(counts[0])
    out = dict.fromkeys(FIT_KEYS, math.nan)
    out['n'] = n
    if n == 0:
        return out
    p, F = model_probabilities(half_range, bins, std, proportions)
    q = np.asarray(hist, dtype=np.float64) / n
    some = q > 0
    with np.errstate(divide='ignore'):
        out['kl'] = math.inf if np.any(p[some] == 0) else float(np.sum(q[some] * np.log(q[some] / p[some])))
    out['tv'] = 0.5 * float(np.sum(np.abs(q - p)))
    cum = np.cumsum(q)
    out['ks'] = max(abs(float(cum[b - 1]) - F[b]) for b in range(1, bins))
    model = p > 0
    out['chi2'] = float(np.sum((q[model] - p[model]) ** 2 / p[model]))
    h = float(half_range)
    s1, s2, s4 = (float(x) for x in sums[:3])
    var_model = sum(pk * s * s for s, pk in zip(std, proportions))
    out['tail'] = int(counts[2]) / n
    out['tail_model'] = sum(pk * math.erfc(h / (s * math.sqrt(2.0))) for s, pk in zip(std, proportions))
    out['mean'] = s1 / n
    out['std'] = math.sqrt(s2 / n)
    out['std_model'] = math.sqrt(var_model)
    out['kurtosis'] = n * s4 / (s2 * s2) if s2 > 0 else math.nan
    out['kurtosis_model'] = 3.0 * sum(pk * s ** 4 for s, pk in zip(std, proportions)) / (var_model * var_model)
    return out


def residual_fit(hist, counts, sums, half_range, std, proportions):
    """The histogram of residual_histogram against the mixture (std, proportions: K numbers each), on the host in float64.
    hist (C,B), counts (C,3), sums (C,4) -- tensors or arrays -- give one dict per chain; (B,), (3,), (4,) give one dict.  With
    q_b = hist_b / n and p_b the mixture's mass in bin b (model_probabilities): 'kl' = sum q ln(q / p) over q > 0 (+inf when
    some p_b = 0 < q_b), 'tv' = 1/2 sum |q - p|, 'ks' = the largest gap of the two cumulative distributions at the interior
    edges, 'chi2' = sum (q - p)^2 / p over p > 0; 'tail' = n_clipped / n against 'tail_model' = the mass beyond +-half_range;
    'mean', 'std' = sqrt(sum z^2 / n) against 'std_model' = sqrt(sum pi sigma^2); 'kurtosis' = n sum z^4 / (sum z^2)^2 against
    'kurtosis_model' = 3 sum pi sigma^4 / (sum pi sigma^2)^2; 'n'.  n == 0: every entry but 'n' is NaN."""
    host = lambda t: np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
    hist, counts, sums = host(hist), host(counts), host(sums)
    std, proportions = _doubles('std', std), _doubles('proportions', proportions)
    if len(std) != len(proportions) or not std:
        raise ValueError(f'residual_fit: {len(std)} scales and {len(proportions)} proportions')
    if hist.ndim == 1:
        return _fit_one(hist, counts, sums, half_range, std, proportions)
    return [_fit_one(hist[c], counts[c], sums[c], half_range, std, proportions) for c in range(hist.shape[0])]
