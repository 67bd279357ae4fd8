"""Convergence diagnostics of the MCMC stage (absent in the reference): split-R-hat, and optionally the split effective
sample size (ESS) and the Monte Carlo standard error (MCSE) of the posterior mean, of the displacement, per voxel.

Each chain's recorded samples are split into two halves (the middle one of an odd count goes to neither), and per half
and chain a Welford mean / M2 is kept on the device (ops.chain_moments_update): 48 * C * D * H * W bytes, whatever the
number of samples.  At the end, ops.split_rhat turns the 2C sequences into the classic split-R-hat of Gelman et al.
(BDA3 section 11.4), the largest over the three displacement components, and a masked summary.

With ESS on, a ring of the last L samples and the lag sums of squared differences (the variogram) are kept as well
(ops.chain_variogram_update): 4 * L * (C + 1) * 3 * D * H * W more bytes.  ops.split_ess turns them and the moments into
BDA3's split ESS (section 11.5) with its truncation rule, and the MCSE sqrt(var+ / ESS).

The posterior label maps (LabelPosterior) follow the same pattern for the propagated segmentation: per-voxel counts of every
structure over the recorded warps (ops.label_posterior_update), 4 * K * D * H * W bytes whatever the number of records, and
at the end the entropy and MAP maps, soft Dice, Dice of the MAP, volume spread and calibration (ops.label_posterior_finalize).

The Jacobian posterior (JacobianPosterior) does the same for the Jacobian determinant of the sampled transformation: per voxel
the number of recorded transformations that fold there and the Welford moments of log det J over the others
(ops.jacobian_posterior_update), 12 * D * H * W bytes whatever the number of records, and at the end the fold probability, the
mean and the std of log det J and their summary over the fixed mask (ops.jacobian_posterior_finalize).

The displacement covariance (DisplacementCovariance) keeps the second moment of the displacement itself, pooled over chains as
the displacement mean / std is: per voxel the Welford mean and the six co-moments (ops.displacement_covariance_update),
36 * D * H * W bytes whatever the number of records, and at the end the principal spreads, the major direction and the
fractional anisotropy of the 3 x 3 sample covariance and their summary over a mask (ops.displacement_covariance_finalize).

The displacement modes (DisplacementModes, displacement_modes_options) are the one summary across voxels, and the one recorder
that keeps the samples: the recorded displacements stay on the device (12 * D * H * W bytes per record, at most max_records of
them) with their per-channel Gram matrix (modes.modes_append), and at the end the host diagonalises the centred, scaled n x n
matrix and one pass over the store forms the mean, the leading 1-sigma mode fields and an explained-variance map
(modes.modes_decompose, modes.modes_project).

The posterior comparison (PosteriorComparison, posterior_comparison_options) keeps two such states, one fed by the VI test
samples and one by the recorded chain samples, 72 * D * H * W bytes, and at the end the distances between the Gaussians they
describe per voxel -- mean shift, log ratio of the total spreads, Bures distance, Jeffreys divergence -- and their summary over
a mask (posterior_comparison.posterior_compare).

The displacement quantiles (DisplacementQuantiles) are what no moment gives: per voxel and channel a histogram of the
displacement around the first record (ops.displacement_quantiles_update), 12 + 6 * bins bytes per voxel whatever the number of
records, and at the end the quantiles of given probabilities, the width of the credible band between the first and the last
and its summary over a mask (ops.displacement_quantiles_finalize).

The inverse consistency (InverseConsistency) checks what a stationary velocity field promises: exp(-v) inverts exp(v).  At a
recorded step it integrates -v (ops.svf_exp_inverse), composes the two maps in both orders (ops.inverse_consistency) and folds
the norm of phi^-1 o phi - id (fixed grid) and of phi o phi^-1 - id (moving grid), in voxels, into a per-voxel Welford mean and
a running maximum (ops.inverse_consistency_update): 16 * D * H * W bytes whatever the number of records.

The landmark posterior (LandmarkPosterior) is the one diagnostic with an independent truth: corresponding landmarks.  At a
recorded step it evaluates the sampled displacement at the K landmarks (ops.transform_points) and folds the mapped points and
their distance to the corresponding points, the target registration error (TRE), into a float64 state of 14 K numbers
(ops.landmark_update); at the end ops.landmark_finalize gives per landmark the TRE statistics, the principal spreads of the
mapped point, its Mahalanobis distance to the truth and the probability integral transform behind the coverage figures.

The Hausdorff option (hausdorff_options) is of another kind: it keeps no state.  It adds the Hausdorff and percentile surface
distances of the propagated segmentation to the point-estimate metrics wherever the ASD is logged.

The native-resolution option (native_resolution_options) keeps no state either: at a logged step it carries the sampled
transformation to the image's own voxel grid (ops.native_warp, native.NativeGrid) and logs Dice and the surface distances there,
in mm under the header zooms.

The intensity-similarity option (image_similarity_options) keeps no state either: at a logged step it compares the fixed image
with the warped moving image the transition produced (ops.image_similarity: joint histogram, MI / NMI, MSE, NCC in one pass) --
the only figures of registration quality that need no segmentation.

The local similarity (LocalSimilarity, local_similarity_options) is the one map that describes the match of intensities and not
the transformation: at a logged step ops.local_similarity gives the windowed LNCC and SSIM of the fixed and the warped moving
image, and at a recorded step the LNCC maps are folded into a per-voxel streaming mean, minimum and count
(ops.local_similarity_update), 12 * D * H * W bytes whatever the number of records.

The surface posterior (SurfacePosterior, surface_posterior_options) is the surface counterpart of the landmark posterior, with
the fixed segmentation as the truth: at a recorded step every voxel of the fixed contour of a structure takes each chain's
signed distance to the same structure's contour in the warped moving segmentation (ops.surface_posterior_update, on the
distances of the Hausdorff call) into a Welford mean and M2, 12 * D * H * W bytes whatever the number of records or structures;
at the end ops.surface_posterior_finalize gives the bias and spread maps and, per structure, the mean signed distance, the
spread and how often the normal band of the samples holds the fixed boundary.

The residual check (ResidualCheck, residual_check_options) is the one diagnostic of the likelihood: at a logged step the
histogram of the masked residuals is set against the mixture that models them (residual_check.py), and at a recorded step the
exact int64 histograms and moment sums are accumulated per chain and -log p(z) under the mixture of that step is folded into a
per-voxel streaming mean (residual_check.residual_nll_update), 8 * D * H * W bytes whatever the number of records.

The image posterior (ImagePosterior, image_posterior_options) carries what a registration exists to move: at a recorded step the
moving image and up to seven more volumes on its grid (a dose or PET map, a second contrast) are sampled under every chain's
transformation and folded into a per-voxel Welford mean / M2, minimum and maximum in one fused launch
(image_posterior.image_posterior_update), 16 * S * D * H * W bytes whatever the number of records; at the end
image_posterior.image_posterior_finalize gives the std and range maps and, for the moving image, the misfit of its posterior mean
against the fixed image in units of the spread the registration uncertainty explains.

The native posterior (NativePosterior, native_posterior_options) puts the label and the image posterior where a user opens them,
on the image's own voxel grid: at a recorded step every chain's displacement is carried to the native grid and the nearest label
and the trilinear sample of the native moving volumes are folded in one fused launch that forms no warped volume
(native_posterior.native_posterior_update), 4 K + 16 bytes per native voxel whatever the number of records; the finalizers of the
label and the image posterior then run on the native extents, with the volumes in mm^3 under the header zooms.

The structure report (StructureReport, structure_report.structure_report_options) is the one recorder that answers per anatomical
structure and the second that keeps a series: at a recorded step one labelled reduction of every chain's displacement and
transformation over the structures of the fixed segmentation (structure_report.structure_motion) writes 11 numbers per chain and
structure into a device series allocated once, 88 * K bytes per record; at the end the host turns the series into the posterior
of every structure's mean displacement and volume change, and the same reduction over the finished maps of the other options
(structure_report.structure_map_stats) gives their per-structure rows.

The truth calibration (TruthCalibration, truth.truth_options) is the one recorder that holds the posterior against an independent
dense truth -- a simulated transformation (truth.known_pair) or a field from elsewhere: at a recorded step one launch counts, per
voxel and channel, the chains below the truth (6 bytes per voxel) and writes every chain's masked error row into a device series,
and a covariance state of its own takes the step; at the end one launch turns state and truth into the error and Mahalanobis
maps, the PIT and rank histograms, the coverage counts and the reliability table.
"""
import math
import numbers
import re

import numpy as np

import torch

from . import _lib as _L
from . import image_posterior as _ip
from . import modes as _modes
from . import ops
from . import posterior_comparison as _pc
from . import residual_check as _rc
from . import structure_report as _sr
from . import truth as _truth


def diagnostics_period(cfg_trainer):
    """`trainer.convergence_diagnostics` -> the recording period P, or None when the option is off.
    Absent / false: off.  true: P = log_period_MCMC.  {"period": P}: that P.  Refuses a config whose chains would give fewer
    than 2 samples per half (N = no_samples_MCMC // P recorded samples per chain, N // 2 per half)."""
    opt = cfg_trainer.get('convergence_diagnostics', False)
    if opt is None or opt is False:
        return None
    if opt is True:
        period = int(cfg_trainer['log_period_MCMC'])
    elif isinstance(opt, dict) and set(opt) <= {'period', 'ess'}:
        period = int(opt.get('period', cfg_trainer['log_period_MCMC']))
    else:
        raise ValueError(f'trainer.convergence_diagnostics must be true, false or {{"period": P, "ess": ...}}, got {opt!r}')
    if period < 1:
        raise ValueError(f'trainer.convergence_diagnostics: the period must be >= 1, got {period}')
    no_samples = int(cfg_trainer['no_samples_MCMC'])
    if no_samples // period // 2 < 2:
        raise ValueError(f'trainer.convergence_diagnostics: no_samples_MCMC = {no_samples} with period {period} records '
                         f'{no_samples // period} samples per chain; split-R-hat needs at least 4 (2 per half)')
    return period


ESS_DEFAULTS = {'max_lag': 32, 'threshold': 400.0}


def _number(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def ess_options(cfg_trainer):
    """`trainer.convergence_diagnostics` -> None when the split ESS is off, else {'max_lag': L, 'threshold': X}.
    Off unless the option is a dict with "ess": true (the defaults, max_lag 32 and threshold 400) or "ess": {"max_lag": L,
    "threshold": X} (either key may be left out).  Refuses max_lag < 3, unknown keys, non-numeric values, and a config whose
    chains would give fewer than 4 samples per half (the truncation rule reads lags 1 to 3)."""
    period = diagnostics_period(cfg_trainer)
    opt = cfg_trainer.get('convergence_diagnostics')
    if period is None or not isinstance(opt, dict):
        return None
    ess = opt.get('ess', False)
    if ess is None or ess is False:
        return None
    out = dict(ESS_DEFAULTS)
    if isinstance(ess, dict):
        unknown = set(ess) - set(ESS_DEFAULTS)
        if unknown:
            raise ValueError(f'trainer.convergence_diagnostics.ess: unknown keys {sorted(unknown)}; '
                             f'known: {sorted(ESS_DEFAULTS)}')
        for key, v in ess.items():
            if not _number(v) or not math.isfinite(v):
                raise ValueError(f'trainer.convergence_diagnostics.ess.{key} must be a finite number, got {v!r}')
        if 'max_lag' in ess:
            if int(ess['max_lag']) != ess['max_lag']:
                raise ValueError(f'trainer.convergence_diagnostics.ess.max_lag must be an integer, got {ess["max_lag"]!r}')
            out['max_lag'] = int(ess['max_lag'])
        if 'threshold' in ess:
            out['threshold'] = float(ess['threshold'])
    elif ess is not True:
        raise ValueError(f'trainer.convergence_diagnostics.ess must be true, false or {{"max_lag": L, "threshold": X}}, '
                         f'got {ess!r}')
    if out['max_lag'] < 3:
        raise ValueError(f'trainer.convergence_diagnostics.ess.max_lag must be >= 3 (the truncation rule reads lags 1 to 3), '
                         f'got {out["max_lag"]}')
    if out['threshold'] <= 0:
        raise ValueError(f'trainer.convergence_diagnostics.ess.threshold must be > 0, got {out["threshold"]}')
    no_samples = int(cfg_trainer['no_samples_MCMC'])
    if no_samples // period // 2 < 4:
        raise ValueError(f'trainer.convergence_diagnostics.ess: no_samples_MCMC = {no_samples} with period {period} records '
                         f'{no_samples // period} samples per chain; the split ESS needs at least 8 (4 per half)')
    return out


def is_recorded(sample_no, no_iters_burn_in, period):
    """the post-burn-in transitions the diagnostic records: (sample_no - burn-in) % period == 0"""
    return sample_no > no_iters_burn_in and (sample_no - no_iters_burn_in) % period == 0


def recorded_steps(no_iters_burn_in, no_samples_MCMC, period):
    """every sample_no the trainer records, in order (no_samples_MCMC // period of them)"""
    first = no_iters_burn_in + 1
    return [s for s in range(first, first + no_samples_MCMC) if is_recorded(s, no_iters_burn_in, period)]


def _bool_mask(mask, device):
    """a mask (or None) on `device` as the bool / uint8 volume the operators take: any other dtype counts where it is != 0"""
    if mask is None:
        return None
    mask = mask.to(device)
    return mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0


def _host_summary(isum, fsum):
    """the int64 and the float64 summary vectors of a finalize in ONE device-to-host copy -> (list of ints, list of floats)"""
    host = torch.cat([isum.view(torch.float64), fsum]).cpu()
    ni = isum.numel()
    return host[:ni].view(torch.int64).tolist(), host[ni:].tolist()


def voxel_scale(dims):
    """normalised coordinates -> voxels, channels x, y, z: (W - 1) / 2, (H - 1) / 2, (D - 1) / 2"""
    D, H, W = dims
    return ((W - 1) / 2, (H - 1) / 2, (D - 1) / 2)


MAX_RECORDS = 2 ** 31 - 1  # the int32 counts


def _record_options(cfg_trainer, key, known, form, ceiling, holds, own_keys=lambda opt: {}):
    """The skeleton the `trainer.<key>` options of the per-voxel recorders share -> None when off, else {'period': P, **own}.
    Absent / false / null: off.  true: P = log_period_MCMC.  A dict of `known` keys: "period" may be left out.  Refuses
    unknown keys, a non-integer P or P < 1, a config that records no step (no_samples_MCMC // P < 1) and one that would
    record more than `ceiling` (`holds`: the words of that message).  `own_keys(dict)` validates the option's other keys
    ({} for true) and returns their values; `form` is how the message for anything else spells the accepted dict."""
    what = f'trainer.{key}'
    opt = cfg_trainer.get(key, False)
    if opt is None or opt is False:
        return None
    period = None
    if isinstance(opt, dict):
        unknown = set(opt) - set(known)
        if unknown:
            raise ValueError(f'{what}: unknown keys {sorted(unknown)}; known: {list(known)}')
        if 'period' in opt:
            p = opt['period']
            if isinstance(p, bool) or not isinstance(p, numbers.Integral):
                raise ValueError(f'{what}.period must be an integer, got {p!r}')
            period = int(p)
    elif opt is not True:
        raise ValueError(f'{what} must be true, false or {form}, got {opt!r}')
    out = {'period': period, **own_keys(opt if isinstance(opt, dict) else {})}
    if period is None:
        out['period'] = period = int(cfg_trainer['log_period_MCMC'])
    if period < 1:
        raise ValueError(f'{what}: the period must be >= 1, got {period}')
    no_samples = int(cfg_trainer['no_samples_MCMC'])
    steps = no_samples // period
    if steps < 1:
        raise ValueError(f'{what}: no_samples_MCMC = {no_samples} with period {period} records no step')
    records = steps * int(cfg_trainer.get('no_chains', 1))
    if records > ceiling:
        raise ValueError(f'{what}: {steps} steps of {cfg_trainer.get("no_chains", 1)} chains are {records} records; '
                         f'{holds.format(ceiling)}')
    return out


class _Recorder:
    """What the per-voxel posterior accumulators share: `records`, the number of samples taken so far, the ceiling
    `record()` checks before `_update(sample)` folds the C samples of one step in, and the guard of what needs a record."""
    noun, max_records, exceed = None, MAX_RECORDS, 'exceed {}'
    records = 0

    def record(self, sample):
        C = sample.shape[0]
        if self.records + C > self.max_records:
            raise ValueError(f'{self.noun}: {self.records} + {C} records {self.exceed.format(self.max_records)}')
        self._update(sample)
        self.records += C

    def _need_records(self, method):
        if self.records < 1:
            raise RuntimeError(f'{type(self).__name__}.{method}: nothing recorded')


class ChainMoments:
    """Per-chain, per-half Welford moments of the displacement and the split-R-hat they give; with `max_lag` set, also the
    online variogram of each half and the split ESS / MCSE.

    `record(displacement)` takes the (C,3,D,H,W) float32 sample of every chain; the i-th call goes to the half
    `schedule(N)[i]` says.  `rhat()` and `ess()` need all N calls."""

    def __init__(self, no_chains, dims, n_per_chain, device, max_lag=None):
        self.no_chains, self.dims, self.n_per_chain = int(no_chains), tuple(int(d) for d in dims), int(n_per_chain)
        if self.n_per_chain // 2 < 2:
            raise ValueError(f'split-R-hat needs at least 4 recorded samples per chain (2 per half), got {self.n_per_chain}')
        self.n = self.n_per_chain // 2
        self.device = device
        self._schedule = self.schedule(self.n_per_chain)
        shape = (2, self.no_chains, 3, *self.dims)
        self.mean = torch.zeros(shape, device=device, dtype=torch.float32)
        self.m2 = torch.zeros(shape, device=device, dtype=torch.float32)
        self.count = 0  # calls of record() so far
        self.max_lag = None if max_lag is None else int(max_lag)
        self.ring, self.vsum = None, None
        if self.max_lag is not None:
            if self.max_lag < 1:
                raise ValueError(f'max_lag must be >= 1, got {self.max_lag}')
            if self.n - 1 < 3:
                raise ValueError(f'the split ESS needs at least 8 recorded samples per chain (4 per half), '
                                 f'got {self.n_per_chain}')
            self.ring = torch.zeros((self.max_lag, self.no_chains, 3, *self.dims), device=device, dtype=torch.float32)
            self.vsum = torch.zeros((self.max_lag, 3, *self.dims), device=device, dtype=torch.float32)

    @staticmethod
    def schedule(N):
        """where the i-th of N recorded samples goes: (half, k), k = samples in that half after it; None for the middle
        sample of an odd N.  Samples 0 .. N//2 - 1 form half 0, the last N//2 half 1."""
        n = N // 2
        out = []
        for i in range(N):
            if i < n:
                out.append((0, i + 1))
            elif i >= N - n:
                out.append((1, i - (N - n) + 1))
            else:
                out.append(None)
        return out

    def record(self, displacement):
        if self.count >= self.n_per_chain:
            raise RuntimeError(f'ChainMoments.record: all {self.n_per_chain} samples are recorded already')
        slot = self._schedule[self.count]
        if slot is not None:
            ops.chain_moments_update(displacement, self.mean, self.m2, *slot)
            if self.max_lag is not None:
                ops.chain_variogram_update(displacement, self.ring, self.vsum, slot[1])
        self.count += 1

    def rhat(self, mask=None, thresholds=(1.01, 1.1)):
        """-> (map (D,H,W) float32 on the device, summary dict).  One device-to-host read (the summary)."""
        if self.count != self.n_per_chain:
            raise RuntimeError(f'ChainMoments.rhat: {self.count} of {self.n_per_chain} samples recorded')
        rhat, s = ops.split_rhat(self.mean, self.m2, self.n, _bool_mask(mask, self.device), thresholds)
        voxels, above0, above1, mx, total = s.tolist()
        voxels = int(voxels)
        summary = {'voxels': voxels, 'max': mx if voxels else float('nan'), 'mean': total / voxels if voxels else float('nan')}
        for t, c in zip(thresholds, (above0, above1)):
            summary[f'above_{t:g}'] = int(c)
            summary[f'frac_above_{t:g}'] = c / voxels if voxels else float('nan')
        return rhat, summary

    def ess(self, mask=None, threshold=400.0):
        """-> (ESS map, MCSE map, both (D,H,W) float32 on the device, summary dict).  One device-to-host read (the summary)."""
        if self.max_lag is None:
            raise RuntimeError('ChainMoments.ess: built without max_lag, so no variogram was kept')
        if self.count != self.n_per_chain:
            raise RuntimeError(f'ChainMoments.ess: {self.count} of {self.n_per_chain} samples recorded')
        ess, mcse, s = ops.split_ess(self.mean, self.m2, self.vsum, self.n, _bool_mask(mask, self.device), threshold)
        voxels, below, truncated, mn, total = s.tolist()
        voxels = int(voxels)
        nan = float('nan')
        summary = {'voxels': voxels, 'min': mn if voxels else nan, 'mean': total / voxels if voxels else nan,
                   f'below_{threshold:g}': int(below), f'frac_below_{threshold:g}': below / voxels if voxels else nan,
                   'truncated': int(truncated), 'frac_truncated': truncated / voxels if voxels else nan}
        return ess, mcse, summary

    def state_dict(self):
        sd = {'mean': self.mean.detach().cpu(), 'm2': self.m2.detach().cpu(), 'count': self.count,
              'n_per_chain': self.n_per_chain}
        if self.max_lag is not None:
            sd.update(ring=self.ring.detach().cpu(), vsum=self.vsum.detach().cpu(), max_lag=self.max_lag)
        return sd

    def load_state_dict(self, sd):
        if int(sd['n_per_chain']) != self.n_per_chain or tuple(sd['mean'].shape) != tuple(self.mean.shape):
            raise ValueError(f'chain moments of {tuple(sd["mean"].shape)} / {int(sd["n_per_chain"])} samples per chain do '
                             f'not match this run ({tuple(self.mean.shape)} / {self.n_per_chain})')
        max_lag = sd.get('max_lag')
        if max_lag != self.max_lag and int(sd['count']) > 0:
            raise ValueError(f'chain moments with ESS max_lag {max_lag} (None: ESS off) after {int(sd["count"])} recorded '
                             f'samples do not match this run (max_lag {self.max_lag})')
        self.mean.copy_(sd['mean'])
        self.m2.copy_(sd['m2'])
        if self.max_lag is not None and max_lag == self.max_lag:
            self.ring.copy_(sd['ring'])
            self.vsum.copy_(sd['vsum'])
        self.count = int(sd['count'])


LABEL_OPTION_KEYS = ('period', 'prob_maps')
LABEL_STRUCTURE_METRICS = ('soft_DSC', 'DSC_MAP', 'vol_mean', 'vol_std', 'uncertain_vol', 'ECE')


def label_posterior_options(cfg_trainer):
    """`trainer.label_posterior` -> None when off, else {'period': P, 'prob_maps': bool}.
    Absent / false / null: off.  true: P = log_period_MCMC.  {"period": P, "prob_maps": bool}: either key may be left out.
    Refuses unknown keys, a non-integer P or P < 1, a non-bool prob_maps, a config that records no step
    (no_samples_MCMC // P < 1) and one that would record more than 2^31 - 1 maps."""
    def own_keys(opt):
        if not isinstance(opt.get('prob_maps', False), bool):
            raise ValueError(f'trainer.label_posterior.prob_maps must be true or false, got {opt["prob_maps"]!r}')
        return {'prob_maps': opt.get('prob_maps', False)}

    return _record_options(cfg_trainer, 'label_posterior', LABEL_OPTION_KEYS, '{"period": P, "prob_maps": bool}', MAX_RECORDS,
                           'the counts hold at most {}', own_keys)


def _nan_div(a, b):
    return a / b if b else float('nan')


def label_summary(raw, volume, n, mask_summary, names, spacing):
    """the derived quantities of DESIGN.md section 6 from the finalize's integer sums (host numpy / floats):
    raw (K, 6 + 3B) int64, volume (K, 2) float64 {mean, M2}, n records, mask_summary {voxels, entropy sum, max, ...},
    spacing (sx, sy, sz) -> {'records', 'voxels', 'entropy_mean', 'entropy_max', 'ECE', 'structures': {name: {soft_DSC,
    DSC_MAP, vol_mean, vol_std, uncertain_vol, ECE}}}"""
    raw = np.asarray(raw, dtype=np.int64)
    volume = np.asarray(volume, dtype=np.float64)
    v = float(np.prod([float(x) for x in spacing]))
    bins = raw[:, 6:].reshape(len(names), -1, 3)  # (K, B, {pairs, sum c, sum y})
    structures = {}
    for j, name in enumerate(names):
        S0, S1, S2, S3, S4, S5 = (int(x) for x in raw[j, :6])
        pairs = int(bins[j, :, 0].sum())
        ece = float(np.abs(bins[j, :, 1] / n - bins[j, :, 2]).sum())
        structures[name] = {'soft_DSC': _nan_div(2.0 * S2, S1 + n * S0), 'DSC_MAP': _nan_div(2.0 * S4, S3 + S0),
                            'vol_mean': float(volume[j, 0]) * v,
                            'vol_std': math.sqrt(float(volume[j, 1]) / max(n - 1, 1)) * v,
                            'uncertain_vol': S5 * v, 'ECE': _nan_div(ece, pairs)}
    pooled = bins.sum(axis=0)
    voxels = int(mask_summary[0])
    return {'records': int(n), 'voxels': voxels,
            'entropy_mean': _nan_div(float(mask_summary[1]), voxels),
            'entropy_max': float(mask_summary[2]) if voxels else float('nan'),
            'ECE': _nan_div(float(np.abs(pooled[:, 1] / n - pooled[:, 2]).sum()), int(pooled[:, 0].sum())),
            'structures': structures}


class LabelPosterior(_Recorder):
    """Per-voxel counts of every structure of `structures_dict` over the recorded warps of the moving segmentation, and the
    Welford moments of each structure's per-record volume, on the device (4 K D H W + 16 K bytes whatever the number of
    records).  `record(seg_warped)` takes the (C,1,D,H,W) int16 maps of one step, chains in order; `finalize` gives the
    entropy and MAP maps and the summary; `probabilities()` the (K,D,H,W) label probabilities."""
    noun = 'label posterior'

    def __init__(self, structures_dict, dims, device):
        self.names = list(structures_dict)
        self.labels = [int(structures_dict[k]) for k in self.names]
        if not 1 <= len(self.labels) <= 64:
            raise ValueError(f'label posterior: 1 to 64 structures, got {len(self.labels)}')
        if len(set(self.labels)) != len(self.labels):
            raise ValueError(f'label posterior: the label values {self.labels} are not distinct')
        self.dims = tuple(int(d) for d in dims)
        self.device = device
        self.counts = torch.zeros((len(self.labels), *self.dims), device=device, dtype=torch.int32)
        self.volume = torch.zeros((len(self.labels), 2), device=device, dtype=torch.float64)

    def _update(self, seg_warped):
        ops.label_posterior_update(seg_warped, self.labels, self.counts, self.volume, self.records)

    def finalize(self, seg_fixed, mask=None, spacing=(1.0, 1.0, 1.0)):
        """-> (entropy (D,H,W) float32, map_label (D,H,W) int16, both on the device, summary dict of label_summary).
        The entropy statistics are over `mask` (the FIXED mask: the maps live on the fixed grid).  One device-to-host read."""
        from . import _lib as L
        self._need_records('finalize')
        entropy, map_label, raw, ms = ops.label_posterior_finalize(self.counts, self.records, self.labels,
                                                                   seg_fixed.to(self.device), _bool_mask(mask, self.device))
        host = torch.cat([raw.reshape(-1).view(torch.float64), ms, self.volume.reshape(-1)]).cpu()
        KC = raw.numel()
        raw_h = host[:KC].view(torch.int64).reshape(raw.shape).numpy()
        ms_h = host[KC:KC + 4].numpy()
        vol_h = host[KC + 4:].reshape(-1, 2).numpy()
        if ms_h[3] != 0:
            raise L.IrsError(f'label posterior: {int(ms_h[3])} voxels hold more than the {self.records} records counted: '
                             f'the counts and the record number disagree')
        summary = label_summary(raw_h, vol_h, self.records, ms_h, self.names,
                                spacing.tolist() if hasattr(spacing, 'tolist') else spacing)
        summary['raw'] = raw_h
        return entropy, map_label, summary

    def probabilities(self):
        """-> (K,D,H,W) float32 on the device: counts / n"""
        self._need_records('probabilities')
        return self.counts.float() / self.records

    def state_dict(self):
        return {'counts': self.counts.detach().cpu(), 'volume': self.volume.detach().cpu(), 'records': self.records,
                'labels': list(self.labels)}

    def load_state_dict(self, sd):
        if [int(x) for x in sd['labels']] != self.labels:
            raise ValueError(f'label posterior of labels {list(sd["labels"])} does not match this run ({self.labels})')
        if tuple(sd['counts'].shape) != tuple(self.counts.shape):
            raise ValueError(f'label posterior of shape {tuple(sd["counts"].shape)} does not match this run '
                             f'({tuple(self.counts.shape)})')
        self.counts.copy_(sd['counts'])
        self.volume.copy_(sd['volume'])
        self.records = int(sd['records'])


JACOBIAN_OPTION_KEYS = ('period',)
JACOBIAN_METRICS = ('fold_prob_max', 'fold_prob_mean', 'folded_voxels', 'always_folded', 'logJ_std_mean', 'logJ_std_max')


def jacobian_posterior_options(cfg_trainer):
    """`trainer.jacobian_posterior` -> None when off, else {'period': P}.
    Absent / false / null: off.  true: P = log_period_MCMC.  {"period": P}: that P (the key may be left out).
    Refuses unknown keys, a non-integer P or P < 1, a config that records no step (no_samples_MCMC // P < 1) and one that
    would record more than 2^31 - 1 transformations."""
    return _record_options(cfg_trainer, 'jacobian_posterior', JACOBIAN_OPTION_KEYS, '{"period": P}', MAX_RECORDS,
                           'the fold counts hold at most {}')


def jacobian_summary(isummary, fsummary, n):
    """the summary of DESIGN.md section 6 from the finalize's reduced columns (host ints / floats): isummary {voxels, folded
    voxels, always folded, fold records}, fsummary {max fold_prob, min / max logJ_mean, sum / max logJ_std}, n records.
    An empty mask gives NaN; so do the logJ entries when no masked voxel has a valid record."""
    voxels, folded, always, fold_records = (int(x) for x in isummary)
    fp_max, lm_min, lm_max, ls_sum, ls_max = (float(x) for x in fsummary)
    valid = voxels - always  # voxels with at least one valid record
    nan = float('nan')
    return {'records': int(n), 'voxels': voxels, 'folded_voxels': folded, 'always_folded': always, 'fold_records': fold_records,
            'fold_prob_max': fp_max if voxels else nan, 'fold_prob_mean': _nan_div(fold_records, int(n) * voxels),
            'logJ_mean_min': lm_min if valid else nan, 'logJ_mean_max': lm_max if valid else nan,
            'logJ_std_mean': _nan_div(ls_sum, valid), 'logJ_std_max': ls_max if valid else nan}


class JacobianPosterior(_Recorder):
    """Per voxel, the number of recorded transformations that fold there and the Welford mean / M2 of log det J over those
    that do not, on the device (12 D H W bytes whatever the number of records).  `record(transformation)` takes the
    (C,3,D,H,W) float32 transformations of one step, chains in order; `finalize` gives the fold probability, the mean and
    the std of log det J, and the summary over a mask."""
    noun = 'Jacobian posterior'

    def __init__(self, dims, device):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 2:
            raise ValueError(f'Jacobian posterior: three dims of at least 2, got {self.dims}')
        self.device = device
        self.folds = torch.zeros(self.dims, device=device, dtype=torch.int32)
        self.mean = torch.zeros(self.dims, device=device, dtype=torch.float32)
        self.m2 = torch.zeros(self.dims, device=device, dtype=torch.float32)

    def _update(self, transformation):
        ops.jacobian_posterior_update(transformation, self.folds, self.mean, self.m2, self.records)

    def finalize(self, mask=None):
        """-> (fold_prob, logJ_mean, logJ_std, all (D,H,W) float32 on the device, summary dict of jacobian_summary).
        One device-to-host read (the summary)."""
        self._need_records('finalize')
        fold_prob, logj_mean, logj_std, isum, fsum = ops.jacobian_posterior_finalize(self.folds, self.mean, self.m2, self.records,
                                                                                    _bool_mask(mask, self.device))
        return fold_prob, logj_mean, logj_std, jacobian_summary(*_host_summary(isum, fsum), self.records)

    def state_dict(self):
        return {'folds': self.folds.detach().cpu(), 'mean': self.mean.detach().cpu(), 'm2': self.m2.detach().cpu(),
                'records': self.records}

    def load_state_dict(self, sd):
        for key in ('folds', 'mean', 'm2'):
            if tuple(sd[key].shape) != self.dims:
                raise ValueError(f'Jacobian posterior of shape {tuple(sd[key].shape)} ({key}) does not match this run '
                                 f'({self.dims})')
        self.folds.copy_(sd['folds'])
        self.mean.copy_(sd['mean'])
        self.m2.copy_(sd['m2'])
        self.records = int(sd['records'])


IMAGE_OPTION_KEYS = ('period', 'volumes', 'reference', 'std_floor', 'save')
IMAGE_DEFAULTS = {'volumes': (), 'reference': True, 'std_floor': None, 'save': True}
IMAGE_MAX_EXTRAS = _ip.MAX_VOLUMES - 1  # the moving image is always carried
IMAGE_METRICS = ('std_mean', 'std_max', 'range_max')  # logged per volume
IMAGE_Z_METRICS = ('z_rms', 'z_gt2', 'z_gt3')  # logged for the moving image against the fixed one
IMAGE_STD_FLOOR_FRACTION = 1e-3  # "std_floor": null -> this fraction of the moving image's intensity range


def image_posterior_options(cfg_trainer):
    """`trainer.image_posterior` -> None when off, else {'period': P, 'volumes': ({'name', 'path'}, ...), 'reference': bool,
    'std_floor': float | None, 'save': bool}.
    Absent / false / null: off.  true: the moving image alone, recorded every log_period_MCMC-th step after the burn-in, its z
    map against the fixed image, the floor of z taken from the moving image's intensity range, the maps written.  A dict sets
    any of "period", "volumes" (at most 7 extra volumes {"name": ..., "path": ...} on the moving image's grid, the names unique,
    of [A-Za-z0-9_]+ and not "moving"), "reference", "std_floor" (a number >= 0, or null) and "save".  Refuses unknown keys, a
    non-integer P or P < 1, a config that records no step (no_samples_MCMC // P < 1) and one that would record more than
    2^31 - 1 samples."""
    what = 'trainer.image_posterior'

    def own_keys(opt):
        own = {**IMAGE_DEFAULTS, **{k: v for k, v in opt.items() if k != 'period'}}
        volumes = own['volumes']
        if not isinstance(volumes, (list, tuple)):
            raise ValueError(f'{what}.volumes must be a list of {{"name": ..., "path": ...}}, got {volumes!r}')
        if len(volumes) > IMAGE_MAX_EXTRAS:
            raise ValueError(f'{what}.volumes: {len(volumes)} entries, at most {IMAGE_MAX_EXTRAS} beside the moving image')
        names = []
        for i, entry in enumerate(volumes):
            if not isinstance(entry, dict) or set(entry) != {'name', 'path'}:
                raise ValueError(f'{what}.volumes[{i}] must be {{"name": ..., "path": ...}}, got {entry!r}')
            name, file_path = entry['name'], entry['path']
            if not isinstance(name, str) or not re.fullmatch(r'[A-Za-z0-9_]+', name):
                raise ValueError(f'{what}.volumes[{i}].name must match [A-Za-z0-9_]+, got {name!r}')
            if name == 'moving':
                raise ValueError(f'{what}.volumes[{i}].name: "moving" names the moving image itself')
            if name in names:
                raise ValueError(f'{what}.volumes[{i}].name: {name!r} is listed twice')
            if not isinstance(file_path, str) or not file_path:
                raise ValueError(f'{what}.volumes[{i}].path must be a file name, got {file_path!r}')
            names.append(name)
        for key in ('reference', 'save'):
            if not isinstance(own[key], bool):
                raise ValueError(f'{what}.{key} must be true or false, got {own[key]!r}')
        floor = own['std_floor']
        if floor is not None and (not _number(floor) or not math.isfinite(floor) or floor < 0):
            raise ValueError(f'{what}.std_floor must be a finite number >= 0 or null, got {floor!r}')
        return {'volumes': tuple({'name': e['name'], 'path': e['path']} for e in volumes), 'reference': own['reference'],
                'std_floor': None if floor is None else float(floor), 'save': own['save']}

    return _record_options(cfg_trainer, 'image_posterior', IMAGE_OPTION_KEYS,
                           '{"period": P, "volumes": [...], "reference": bool, "std_floor": x, "save": bool}', MAX_RECORDS,
                           'the sample count holds at most {}', own_keys)


def image_posterior_names(options):
    """the volumes the option carries, in state order: the moving image, then the extras"""
    return ['moving'] + [v['name'] for v in options['volumes']]


def image_posterior_metric_names(options):
    """the metric names the option adds: MCMC/image/{name}/{std_mean,std_max,range_max} per volume and, with "reference",
    MCMC/image/moving/{z_rms,z_gt2,z_gt3}"""
    m = [f'MCMC/image/{name}/{k}' for name in image_posterior_names(options) for k in IMAGE_METRICS]
    return m + ([f'MCMC/image/moving/{k}' for k in IMAGE_Z_METRICS] if options['reference'] else [])


def image_summary(isummary, fsummary, n, with_z):
    """the summary of one volume from the finalize's reduced columns (host ints / floats): isummary {voxels, non-finite voxels,
    |z| > 2, |z| > 3}, fsummary {sum mean, sum / max std, max range, sum z^2, max |z|} over the finite ones, n records.  The
    z entries (`with_z`) are fractions of the finite voxels and the root mean square; an empty mask gives NaN."""
    voxels, nonfinite, gt2, gt3 = (int(x) for x in isummary)
    mean_sum, std_sum, std_max, range_max, z2_sum, z_max = (float(x) for x in fsummary)
    some = voxels - nonfinite
    nan = float('nan')
    out = {'records': int(n), 'voxels': voxels, 'nonfinite_voxels': nonfinite, 'mean': _nan_div(mean_sum, some),
           'std_mean': _nan_div(std_sum, some), 'std_max': std_max if some else nan, 'range_max': range_max if some else nan}
    if with_z:
        out.update(z_rms=math.sqrt(z2_sum / some) if some else nan, z_max=z_max if some else nan, z_gt2=_nan_div(gt2, some),
                   z_gt3=_nan_div(gt3, some))
    return out


class ImagePosterior(_Recorder):
    """Per voxel of the fixed grid and volume, the Welford mean / M2, the minimum and the maximum of the volume's trilinear sample
    under every recorded transformation, on the device (16 S D H W bytes whatever the number of records).  `volumes`
    (S,1,D,H,W) float32 live on the moving image's grid and are shared by the chains; `names`: one per volume.
    `record(transformation)` takes the (C,3,D,H,W) float32 transformations of one step, chains in order, in ONE launch for all
    volumes; `finalize` gives every volume's maps and summary."""
    noun = 'image posterior'

    def __init__(self, volumes, names, device):
        names = tuple(str(n) for n in names)
        if volumes.dim() != 5 or volumes.shape[1] != 1 or volumes.shape[0] != len(names) or len(set(names)) != len(names):
            raise ValueError(f'image posterior: (S,1,D,H,W) volumes and S distinct names, got {tuple(volumes.shape)} and {names}')
        self.names, self.device = names, device
        self.dims = tuple(int(d) for d in volumes.shape[2:])
        self.volumes = volumes.to(device=device, dtype=torch.float32).contiguous()
        self.state = _ip.image_posterior_state(len(names), self.dims, device)

    def _update(self, transformation):
        _ip.image_posterior_update(self.volumes, transformation, self.state, self.records)

    def finalize(self, mask=None, reference=None, std_floor=0.0):
        """-> {name: {'mean', 'std', 'range' (D,H,W) float32 on the device[, 'z'], 'summary': image_summary}}.  reference:
        {name: volume on the fixed grid} or None: those volumes get a z map, (reference - mean) / sqrt(std^2 + std_floor^2).
        One device-to-host read per volume (the summary)."""
        self._need_records('finalize')
        reference = dict(reference or {})
        unknown = set(reference) - set(self.names)
        if unknown:
            raise ValueError(f'image posterior: reference for {sorted(unknown)}, the volumes are {list(self.names)}')
        mask = _bool_mask(mask, self.device)
        out = {}
        for index, name in enumerate(self.names):
            ref = reference.get(name)
            ref = None if ref is None else ref.to(device=self.device, dtype=torch.float32)
            std, rng, z, isum, fsum = _ip.image_posterior_finalize(self.state, index, self.records, ref, std_floor, mask)
            nan = std.new_full((), math.nan)
            mean = self.state['mean'][index]
            out[name] = {'mean': mean.where(mean.isfinite(), nan), 'std': std, 'range': rng,
                         'summary': image_summary(*_host_summary(isum, fsum), self.records, ref is not None)}
            if z is not None:
                out[name]['z'] = z
        return out

    def state_dict(self):
        return {'records': self.records, 'names': list(self.names), 'dims': list(self.dims),
                **{key: t.detach().cpu() for key, t in self.state.items()}}

    def load_state_dict(self, sd):
        if tuple(sd['names']) != self.names:
            raise ValueError(f'image posterior of the volumes {list(sd["names"])} does not match this run ({list(self.names)})')
        if tuple(sd['dims']) != self.dims:
            raise ValueError(f'image posterior of dims {tuple(sd["dims"])} does not match this run ({self.dims})')
        for key, t in self.state.items():
            if tuple(sd[key].shape) != tuple(t.shape):
                raise ValueError(f'image posterior state of shape {tuple(sd[key].shape)} ({key}) does not match this run '
                                 f'({tuple(t.shape)})')
        for key, t in self.state.items():
            t.copy_(sd[key])
        self.records = int(sd['records'])


COVARIANCE_OPTION_KEYS = ('period',)
COVARIANCE_METRICS = ('std_major_mean', 'std_major_max', 'std_total_mean', 'anisotropy_mean', 'anisotropy_max', 'dir_x', 'dir_y',
                      'dir_z')


def displacement_covariance_options(cfg_trainer):
    """`trainer.displacement_covariance` -> None when off, else {'period': P}.
    Absent / false / null: off.  true: P = log_period_MCMC.  {"period": P}: that P (the key may be left out).
    Refuses unknown keys, a non-integer P or P < 1, a config that records no step (no_samples_MCMC // P < 1) and one that
    would record more than 2^31 - 1 displacements."""
    return _record_options(cfg_trainer, 'displacement_covariance', COVARIANCE_OPTION_KEYS, '{"period": P}', MAX_RECORDS,
                           'the record count holds at most {}')


def covariance_summary(isummary, fsummary, n):
    """the summary of DESIGN.md section 6 from the finalize's reduced columns (host ints / floats): isummary {voxels, voxels
    with a non-finite state}, fsummary {sum / max std[0], sum of the total std, sum / max anisotropy, sums of |direction_c|}
    over the finite masked voxels, n records.  The float entries are NaN for an empty mask or when no masked voxel is finite;
    dir_x / dir_y / dir_z are the mean absolute components of the major direction: which axis carries the uncertainty."""
    voxels, nonfinite = (int(x) for x in isummary)
    s_sum, s_max, t_sum, a_sum, a_max, dx, dy, dz = (float(x) for x in fsummary)
    finite = voxels - nonfinite
    nan = float('nan')
    return {'records': int(n), 'voxels': voxels, 'nonfinite_voxels': nonfinite,
            'std_major_mean': _nan_div(s_sum, finite), 'std_major_max': s_max if finite else nan,
            'std_total_mean': _nan_div(t_sum, finite), 'anisotropy_mean': _nan_div(a_sum, finite),
            'anisotropy_max': a_max if finite else nan,
            'dir_x': _nan_div(dx, finite), 'dir_y': _nan_div(dy, finite), 'dir_z': _nan_div(dz, finite)}


class DisplacementCovariance(_Recorder):
    """Per voxel, the Welford mean (3,D,H,W) and the co-moments (6,D,H,W: xx, yy, zz, xy, xz, yz) of the displacement over the
    recorded samples, pooled over chains, on the device (36 D H W bytes whatever the number of records).
    `record(displacement)` takes the (C,3,D,H,W) float32 displacements of one step, chains in order; `finalize` gives the
    principal standard deviations, the major direction, the fractional anisotropy and the summary over a mask."""
    noun = 'displacement covariance'

    def __init__(self, dims, device):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 2:
            raise ValueError(f'displacement covariance: three dims of at least 2, got {self.dims}')
        self.device = device
        self.mean = torch.zeros((3,) + self.dims, device=device, dtype=torch.float32)
        self.comoment = torch.zeros((6,) + self.dims, device=device, dtype=torch.float32)

    def default_scale(self):
        return voxel_scale(self.dims)

    def _update(self, displacement):
        ops.displacement_covariance_update(displacement, self.mean, self.comoment, self.records)

    def covariance(self):
        """-> (6,D,H,W) float32: the sample covariance in normalised units, comoment / max(n - 1, 1)"""
        self._need_records('covariance')
        return self.comoment / max(self.records - 1, 1)

    def finalize(self, mask=None, scale=None):
        """-> (std (3,D,H,W), direction (3,D,H,W), anisotropy (D,H,W), float32 on the device, summary dict of
        covariance_summary).  scale: three positive floats, one per channel (default: voxel units).  One device-to-host
        read (the summary)."""
        self._need_records('finalize')
        scale = self.default_scale() if scale is None else tuple(float(s) for s in scale)
        std, direction, anisotropy, isum, fsum = ops.displacement_covariance_finalize(self.mean, self.comoment, self.records,
                                                                                      scale, _bool_mask(mask, self.device))
        return std, direction, anisotropy, covariance_summary(*_host_summary(isum, fsum), self.records)

    def state_dict(self):
        return {'mean': self.mean.detach().cpu(), 'comoment': self.comoment.detach().cpu(), 'records': self.records}

    def load_state_dict(self, sd):
        for key, ch in (('mean', 3), ('comoment', 6)):
            if tuple(sd[key].shape) != (ch,) + self.dims:
                raise ValueError(f'displacement covariance of shape {tuple(sd[key].shape)} ({key}) does not match this run '
                                 f'({(ch,) + self.dims})')
        self.mean.copy_(sd['mean'])
        self.comoment.copy_(sd['comoment'])
        self.records = int(sd['records'])


MODES_OPTION_KEYS = ('period', 'modes', 'max_records', 'save')
MODES_DEFAULTS = {'modes': 8, 'max_records': 256, 'save': True}
MODES_METRICS = ('var_total', 'explained_1', 'explained_M', 'n90', 'participation', 'std_1', 'rhat_max')


def displacement_modes_options(cfg_trainer):
    """`trainer.displacement_modes` -> None when off, else {'period': P, 'modes': M, 'max_records': cap, 'save': bool}.
    Absent / false / null: off.  true: the defaults (P = log_period_MCMC, 8 modes, a store of 256 records, save).  A dict: any of
    "period", "modes" (1 .. 16), "max_records" (2 .. 1024: the records the device store holds, 12 D H W bytes each) and "save"
    (write the mode fields and the explained map with save_outputs).  Refuses unknown keys, wrong types (booleans as numbers
    too), values out of range, a config that records no step or fewer than 2 records in all, and one that would record more
    than max_records (nothing is thinned or dropped: raise max_records or the period)."""
    what = 'trainer.displacement_modes'

    def own_keys(opt):
        out = dict(MODES_DEFAULTS)
        for key, lo, hi in (('modes', 1, _L.IRS_MODES_MAX), ('max_records', 2, _L.IRS_MODES_MAX_RECORDS)):
            if key in opt:
                v = opt[key]
                if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                    raise ValueError(f'{what}.{key} must be an integer, got {v!r}')
                if not lo <= v <= hi:
                    raise ValueError(f'{what}.{key} must be in {lo} .. {hi}, got {v}')
                out[key] = int(v)
        if 'save' in opt and not isinstance(opt['save'], bool):
            raise ValueError(f'{what}.save must be true or false, got {opt["save"]!r}')
        out['save'] = opt.get('save', True)
        return out

    opt = cfg_trainer.get('displacement_modes', False)
    if opt is None or opt is False:
        return None
    # the ceiling is the option's own max_records: read it first (own_keys runs again inside, after the key checks)
    ceiling = MODES_DEFAULTS['max_records']
    if isinstance(opt, dict) and not (set(opt) - set(MODES_OPTION_KEYS)):
        ceiling = own_keys(opt)['max_records']
    out = _record_options(cfg_trainer, 'displacement_modes', MODES_OPTION_KEYS,
                          '{"period": P, "modes": M, "max_records": N, "save": true}', ceiling,
                          'the store holds at most {} (trainer.displacement_modes.max_records; nothing is thinned)', own_keys)
    records = int(cfg_trainer['no_samples_MCMC']) // out['period'] * int(cfg_trainer.get('no_chains', 1))
    if records < 2:
        raise ValueError(f'{what}: the run records {records} displacement; modes need at least 2')
    return out


def modes_summary(dec, M):
    """the summary of DESIGN.md section 6 from modes.modes_decompose's dict: records, modes kept, var_total (voxels^2 summed over
    the mask), explained_1 and explained_M (the share of the first mode and of the first M together), n90, the participation
    ratio, std_1 (RMS voxel displacement of the first mode) and rhat_max (the largest split-R-hat of the M score series; NaN
    with one chain or fewer than 4 records per chain)"""
    K = min(int(M), len(dec['eigenvalues']))
    rhat = dec['rhat'][:K]
    finite = rhat[~np.isnan(rhat)]
    return {'records': int(dec['n']), 'modes': K, 'var_total': float(dec['var_total']),
            'explained_1': float(dec['explained'][0]) if K else float('nan'),
            'explained_M': float(np.sum(dec['explained'][:K])) if K else float('nan'), 'n90': int(dec['n90']),
            'participation': float(dec['participation']), 'std_1': float(dec['std'][0]) if K else float('nan'),
            'rhat_max': float(finite.max()) if finite.size else float('nan')}


class DisplacementModes(_Recorder):
    """The recorded displacements themselves, on the device, and their Gram matrix (modes.py): `record(displacement)` takes the
    (C,3,D,H,W) float32 displacements of one step, chains in order, into the next C slots of a store of `cap` records (12 D H W
    cap bytes) and fills their rows of the per-channel Gram matrices; `finalize(M)` diagonalises the centred, scaled Gram matrix
    on the host and forms the mean, the M leading 1-sigma mode fields and the explained-variance map in one pass over the
    store.  The mask is fixed at creation: it enters the Gram matrix (the inner product of the modes) only."""
    noun = 'displacement modes'
    exceed = 'exceed the store of {} (trainer.displacement_modes.max_records)'

    def __init__(self, dims, device, cap, mask=None, logger=None):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 2:
            raise ValueError(f'displacement modes: three dims of at least 2, got {self.dims}')
        self.device, self.cap, self.max_records, self.logger = device, int(cap), int(cap), logger
        self.dev = _modes.modes_state(self.dims, self.cap, device, _bool_mask(mask, device))
        self.steps, self.chains = [], []
        self._logged_checkpoint = False
        if logger is not None:
            logger.info(f'displacement modes: a store of {self.cap} records, {self.store_bytes() / 1e6:.1f} MB on the device '
                        f'(12 x {int(np.prod(self.dims))} voxels x {self.cap}), {self.dev["mask_voxels"]} voxels in the mask')

    def store_bytes(self):
        return 12 * int(np.prod(self.dims)) * self.cap

    def default_scale(self):
        return voxel_scale(self.dims)

    def record(self, sample, step=None):
        C = sample.shape[0]
        super().record(sample)
        step = (self.steps[-1] + 1 if self.steps else 1) if step is None else int(step)
        self.steps += [step] * C
        self.chains += list(range(C))

    def _update(self, displacement):
        _modes.modes_append(self.dev, displacement)

    def gram(self):
        return _modes.modes_gram(self.dev)

    def finalize(self, M=MODES_DEFAULTS['modes'], scale=None):
        """-> {'eigenvalues', 'explained', 'scores', 'rhat' (numpy, of modes_decompose), 'mean' (3,D,H,W), 'modes' (K,3,D,H,W):
        the 1-sigma mode fields in normalised coordinates, 'explained_map' (D,H,W), float32 on the device, 'steps', 'chains',
        'summary': modes_summary}, K = min(M, n - 1).  Needs at least 2 records.  One device-to-host read (the Gram matrix)."""
        self._need_records('finalize')
        if self.records < 2:
            raise RuntimeError(f'DisplacementModes.finalize: {self.records} record; modes need at least 2')
        if isinstance(M, bool) or not isinstance(M, numbers.Integral) or not 1 <= M <= _L.IRS_MODES_MAX:
            raise ValueError(f'displacement modes: M must be an integer in 1 .. {_L.IRS_MODES_MAX}, got {M!r}')
        scale = self.default_scale() if scale is None else tuple(float(s) for s in scale)
        dec = _modes.modes_decompose(self.gram(), scale, self.dev['mask_voxels'], self.chains, M)
        mean, fields, explained_map = _modes.modes_project(self.dev, dec['coeff'], scale)
        return {'eigenvalues': dec['eigenvalues'], 'explained': dec['explained'], 'scores': dec['scores'], 'rhat': dec['rhat'],
                'mean': mean, 'modes': fields, 'explained_map': explained_map, 'steps': list(self.steps), 'chains': list(self.chains),
                'summary': modes_summary(dec, M)}

    def state_dict(self):
        n = self.records
        sd = {'store': self.dev['store'][:n].detach().cpu(), 'gram': self.dev['gram'].detach().cpu(), 'records': n, 'cap': self.cap,
              'steps': list(self.steps), 'chains': list(self.chains)}
        if self.logger is not None and not self._logged_checkpoint:
            self._logged_checkpoint = True
            self.logger.info(f'displacement modes: a checkpoint holds the {n} records so far, {12 * int(np.prod(self.dims)) * n / 1e6:.1f} '
                             f'MB now and up to {self.store_bytes() / 1e6:.1f} MB')
        return sd

    def load_state_dict(self, sd):
        n = int(sd['records'])
        if tuple(sd['store'].shape) != (n, 3) + self.dims:
            raise ValueError(f'displacement modes of shape {tuple(sd["store"].shape)} (store) do not match this run '
                             f'({(n, 3) + self.dims})')
        if int(sd['cap']) != self.cap or tuple(sd['gram'].shape) != (3, self.cap, self.cap):
            raise ValueError(f'displacement modes with a store of {int(sd["cap"])} records do not match this run '
                             f'(trainer.displacement_modes.max_records = {self.cap})')
        self.dev['store'][:n].copy_(sd['store'])
        self.dev['gram'].copy_(sd['gram'])
        self.dev['n'] = self.records = n
        self.steps, self.chains = [int(s) for s in sd['steps']], [int(c) for c in sd['chains']]


class StructureReport(_Recorder):
    """Per structure of the fixed segmentation, the series of the per-record sums behind the posterior of its mean displacement
    and of its volume change (structure_report.py): two device arrays, (steps * C, K, 2) int64 and (steps * C, K, 9) float64,
    allocated once -- the number of records is known from the config -- and written row by row.  `record((displacement,
    transformation))` takes the (C,3,D,H,W) float32 outputs of one step, chains in order, and one launch writes rows records ..
    records + C of both; `finalize` copies the series to the host once and gives the per-structure table."""
    noun = 'structure report'
    exceed = 'exceed the {} rows the series was allocated for'

    def __init__(self, seg_fixed, structures_dict, capacity, device, scale=(1.0, 1.0, 1.0), mask=None):
        if seg_fixed.dim() < 3 or seg_fixed.numel() != int(np.prod(seg_fixed.shape[-3:])):
            raise ValueError(f'structure report: seg_fixed must be one (D,H,W) volume, got {tuple(seg_fixed.shape)}')
        self.dims = tuple(int(d) for d in seg_fixed.shape[-3:])
        if min(self.dims) < 2:
            raise ValueError(f'structure report: three dims of at least 2, got {self.dims}')
        if not structures_dict:
            raise ValueError('structure report: structures_dict is empty')
        self.names, self.labels = list(structures_dict), [int(v) for v in structures_dict.values()]
        if len(self.labels) > _L.IRS_MAX_LABELS:
            raise ValueError(f'structure report: {len(self.labels)} structures, at most {_L.IRS_MAX_LABELS}')
        self.device, self.max_records = device, int(capacity)
        if self.max_records < 1:
            raise ValueError(f'structure report: room for {capacity} records, at least 1 needed')
        self.scale = tuple(float(s) for s in scale)
        self.seg_fixed = seg_fixed.reshape(self.dims).to(device=device, dtype=torch.int16).contiguous()
        self.mask = _bool_mask(mask, device)
        K = len(self.labels)
        self.ints = torch.zeros((self.max_records, K, _L.IRS_STRUCTURE_MOTION_INTS), device=device, dtype=torch.int64)
        self.floats = torch.zeros((self.max_records, K, _L.IRS_STRUCTURE_MOTION_FLOATS), device=device, dtype=torch.float64)

    def record(self, sample):
        displacement, transformation = sample
        if tuple(displacement.shape) != tuple(transformation.shape):
            raise ValueError(f'structure report: displacement {tuple(displacement.shape)} and transformation '
                             f'{tuple(transformation.shape)} differ in shape')
        C = displacement.shape[0]
        if self.records + C > self.max_records:
            raise ValueError(f'{self.noun}: {self.records} + {C} records {self.exceed.format(self.max_records)}')
        self._update(displacement, transformation)
        self.records += C

    def _update(self, displacement, transformation):
        rows = slice(self.records, self.records + displacement.shape[0])
        _sr.structure_motion(displacement, transformation, self.seg_fixed, self.labels, self.scale, self.mask,
                             out=(self.ints[rows], self.floats[rows]))

    def series(self):
        """-> (ints (records,K,2) int64, floats (records,K,9) float64) as numpy: ONE device-to-host copy"""
        self._need_records('series')
        both = torch.cat([self.ints[:self.records].view(torch.float64), self.floats[:self.records]], dim=2).cpu()
        ni = _L.IRS_STRUCTURE_MOTION_INTS
        return both[..., :ni].contiguous().view(torch.int64).numpy(), both[..., ni:].contiguous().numpy()

    def map_stats(self, maps):
        """structure_report.structure_map_stats of (M,D,H,W) float32 maps over this report's structures, on the device"""
        return _sr.structure_map_stats(maps, self.seg_fixed, self.labels, self.mask)

    def finalize(self, spacing=(1.0, 1.0, 1.0), chains=1, cov_trace=None):
        """-> (summary dict of structure_report.structure_summary, (ints, floats) of series())"""
        ints, floats = self.series()
        return _sr.structure_summary(ints, floats, self.names, spacing, chains, cov_trace), (ints, floats)

    def state_dict(self):
        return {'ints': self.ints.detach().cpu(), 'floats': self.floats.detach().cpu(), 'records': self.records}

    def load_state_dict(self, sd):
        for key, t in (('ints', self.ints), ('floats', self.floats)):
            if tuple(sd[key].shape) != tuple(t.shape):
                raise ValueError(f'structure report series of shape {tuple(sd[key].shape)} ({key}) does not match this run '
                                 f'({tuple(t.shape)})')
        self.ints.copy_(sd['ints'])
        self.floats.copy_(sd['floats'])
        self.records = int(sd['records'])


class TruthCalibration(_Recorder):
    """The recorded displacement against a dense truth (truth.py): `below` (3,D,H,W) uint16, per voxel and channel the number of
    records strictly below the truth; a displacement covariance state of its own; and a device series of the per-record error
    rows, (steps * C, 2) int64 and (steps * C, 3) float64, allocated once.  truth: (3,D,H,W) float32 in the unit of the recorded
    displacement (voxels of the registration grid for the trainer's); scale: three positive floats, one per channel, the unit
    of the errors (default 1: that of the displacement); mask: the voxels the series and, by default, the summary are taken
    over.  `record(displacement)` takes the (C,3,D,H,W) float32 displacements of one step, chains in order: one launch of
    truth.truth_update and one of the covariance update; `finalize` gives the maps, the tables and the summary with one
    device-to-host read."""
    noun, max_records, exceed = 'truth calibration', _L.IRS_TRUTH_MAX_RECORDS, 'exceed the {} a uint16 rank count holds'

    def __init__(self, truth, capacity, device, scale=(1.0, 1.0, 1.0), mask=None):
        if truth.dim() != 4 or truth.shape[0] != 3:
            raise ValueError(f'truth calibration: the truth must have shape (3,D,H,W), got {tuple(truth.shape)}')
        self.dims = tuple(int(d) for d in truth.shape[1:])
        if min(self.dims) < 2:
            raise ValueError(f'truth calibration: three dims of at least 2, got {self.dims}')
        self.capacity = int(capacity)
        if not 1 <= self.capacity <= self.max_records:
            raise ValueError(f'truth calibration: room for {capacity} records, 1..{self.max_records} needed')
        self.device = device
        self.scale = tuple(float(s) for s in scale)
        if len(self.scale) != 3 or not all(math.isfinite(s) and s > 0 for s in self.scale):
            raise ValueError(f'truth calibration: scale must hold three finite floats > 0, got {scale}')
        self.truth = truth.to(device=device, dtype=torch.float32).contiguous()
        self.fingerprint = _truth.fingerprint(self.truth)
        self.mask = _bool_mask(mask, device)
        self.below = _truth.new_below(self.dims, device)
        self.covariance = DisplacementCovariance(self.dims, device)
        self.ints = torch.zeros((self.capacity, _L.IRS_TRUTH_UPDATE_INTS), device=device, dtype=torch.int64)
        self.floats = torch.zeros((self.capacity, _L.IRS_TRUTH_UPDATE_FLOATS), device=device, dtype=torch.float64)
        self.workspace = _truth.TruthWorkspace(device)

    def record(self, displacement):
        C = displacement.shape[0]
        if self.records + C > self.capacity:
            raise ValueError(f'{self.noun}: {self.records} + {C} records exceed the {self.capacity} rows the series was allocated for')
        super().record(displacement)

    def _update(self, displacement):
        rows = slice(self.records, self.records + displacement.shape[0])
        _truth.truth_update(displacement, self.truth, self.below, self.records, self.scale, self.mask,
                            out=(self.ints[rows], self.floats[rows]), workspace=self.workspace)
        self.covariance.record(displacement)

    def initial_error(self):
        """{'mean', 'rmse', 'max'} of the error of the identity -- a zero displacement -- over the mask: the update kernel into
        scratch state.  One device-to-host read."""
        zero = torch.zeros((1, 3) + self.dims, device=self.device, dtype=torch.float32)
        ints, floats = _truth.truth_update(zero, self.truth, _truth.new_below(self.dims, self.device), 0, self.scale, self.mask,
                                           workspace=self.workspace)
        return _truth.error_stats(*_host_summary(ints.reshape(-1), floats.reshape(-1)))

    def finalize(self, mask=None, levels=(0.5, 0.9, 0.95), pit_bins=20, rank_bins=16, reliability_bins=16, std_floor=1e-3,
                 reference='hotelling', initial=None, floor=None):
        """mask: the voxels of the summary and the tables (None: the recorder's own).  -> ({'error', 'mahalanobis'}: (D,H,W)
        float32 maps on the device, summary dict of truth.calibration_summary, (ints, floats): the series as numpy arrays).
        One device-to-host read: tables, summary and series travel together."""
        self._need_records('finalize')
        n = self.records
        if n < _truth.MIN_RECORDS[reference]:
            raise RuntimeError(f'TruthCalibration.finalize: {n} records, at least {_truth.MIN_RECORDS[reference]} needed with the '
                               f'{reference!r} reference')
        d2_edges, level_d2 = _truth.calibration_thresholds(n, levels, pit_bins, reference)
        var_edges = _truth.default_var_edges(reliability_bins)
        mask = self.mask if mask is None else _bool_mask(mask, self.device)
        res = _truth.truth_calibrate(self.covariance.mean, self.covariance.comoment, self.below, self.truth, n, self.scale, d2_edges,
                                     level_d2, rank_bins, var_edges, std_floor, mask, workspace=self.workspace)
        parts_i = [res['isummary'], res['counts'], res['rel_ints'].reshape(-1), self.ints[:n].reshape(-1)]
        parts_f = [res['fsummary'], res['rel_floats'].reshape(-1), self.floats[:n].reshape(-1)]
        host = torch.cat([torch.cat(parts_i).view(torch.float64), torch.cat(parts_f)]).cpu()
        ni = sum(p.numel() for p in parts_i)
        hi, hf = host[:ni].contiguous().view(torch.int64).numpy(), host[ni:].numpy()
        cut = lambda arr, parts: np.split(arr, np.cumsum([p.numel() for p in parts])[:-1])
        isummary, counts, rel_ints, ints = cut(hi, parts_i)
        fsummary, rel_floats, floats = cut(hf, parts_f)
        B, Lv = int(pit_bins), len(level_d2)
        summary = _truth.calibration_summary(isummary, fsummary, counts[:B], counts[B:B + Lv], counts[B + Lv:].reshape(3, -1), rel_ints,
                                             rel_floats.reshape(-1, 2), n, levels, reference, var_edges, initial, floor)
        return ({'error': res['error'], 'mahalanobis': res['mahalanobis']}, summary,
                (ints.reshape(n, -1).copy(), floats.reshape(n, -1).copy()))

    def state_dict(self):
        return {'below': self.below.detach().cpu(), 'covariance': self.covariance.state_dict(), 'ints': self.ints.detach().cpu(),
                'floats': self.floats.detach().cpu(), 'records': self.records, 'fingerprint': self.fingerprint}

    def load_state_dict(self, sd):
        if sd['fingerprint'] != self.fingerprint:
            raise ValueError(f'truth calibration: the checkpoint was recorded against another truth (fingerprint '
                             f'{str(sd["fingerprint"])[:12]}..., this run {self.fingerprint[:12]}...)')
        for key, t in (('below', self.below), ('ints', self.ints), ('floats', self.floats)):
            if tuple(sd[key].shape) != tuple(t.shape) or sd[key].dtype != t.dtype:
                raise ValueError(f'truth calibration state of shape {tuple(sd[key].shape)} {sd[key].dtype} ({key}) does not match '
                                 f'this run ({tuple(t.shape)} {t.dtype})')
        records = int(sd['records'])
        if not 0 <= records <= self.capacity or int(sd['covariance']['records']) != records:
            raise ValueError(f'truth calibration: {records} records ({sd["covariance"]["records"]} in the covariance state), 0..'
                             f'{self.capacity} expected')
        self.below.view(torch.int16).copy_(sd['below'].view(torch.int16))
        self.ints.copy_(sd['ints'])
        self.floats.copy_(sd['floats'])
        self.covariance.load_state_dict(sd['covariance'])
        self.records = records


COMPARISON_OPTION_KEYS = ('period', 'std_floor')
COMPARISON_MIN_RECORDS = 4  # a 3 x 3 covariance of fewer than four samples is singular by construction
COMPARISON_METRICS = ('shift_mean', 'shift_max', 'log_std_ratio_mean', 'log_std_ratio_min', 'log_std_ratio_max', 'std_ratio',
                      'frac_vi_narrower', 'bures_mean', 'bures_max', 'w2_mean', 'w2_max', 'jeffreys_mean', 'jeffreys_max',
                      'std_total_vi', 'std_total_mcmc')


def posterior_comparison_options(cfg_trainer):
    """`trainer.posterior_comparison` -> None when off, else {'period': P, 'std_floor': f}.
    Absent / false / null: off.  true: P = log_period_MCMC, f = 1e-3.  A dict: either key may be left out.  The floor is in
    the units of the comparison's scale (voxels).  Refuses what _record_options refuses, a floor that is not a finite number
    > 0, `MCMC: false`, `VI: false` unless `resume` is set (the VI side then comes from the checkpoint), and fewer than 4
    records on either side: no_samples_VI_test < 4, or (no_samples_MCMC // P) * no_chains < 4."""
    what = 'trainer.posterior_comparison'

    def own_keys(opt):
        f = opt.get('std_floor', 1e-3)
        if not _number(f) or not math.isfinite(f) or not f > 0:
            raise ValueError(f'{what}.std_floor must be a finite number > 0, got {f!r}')
        return {'std_floor': float(f)}

    out = _record_options(cfg_trainer, 'posterior_comparison', COMPARISON_OPTION_KEYS, '{"period": P, "std_floor": f}', MAX_RECORDS,
                          'the record count holds at most {}', own_keys)
    if out is None:
        return None
    if not cfg_trainer.get('MCMC', True):
        raise ValueError(f'{what} needs the MCMC stage: MCMC is false')
    vi = bool(cfg_trainer.get('VI', False))
    if not vi and not cfg_trainer.get('resume'):
        raise ValueError(f'{what} needs the VI stage: VI is false and there is no resume checkpoint to take the VI side from')
    need = COMPARISON_MIN_RECORDS
    if vi and int(cfg_trainer['no_samples_VI_test']) < need:
        raise ValueError(f'{what}: no_samples_VI_test = {int(cfg_trainer["no_samples_VI_test"])} records on the VI side, at least '
                         f'{need} needed (a 3 x 3 covariance of fewer samples is singular)')
    no_samples, chains = int(cfg_trainer['no_samples_MCMC']), int(cfg_trainer.get('no_chains', 1))
    steps = no_samples // out['period']
    if steps * chains < need:
        raise ValueError(f'{what}: no_samples_MCMC = {no_samples} with period {out["period"]} gives {steps} steps of {chains} chains: '
                         f'{steps * chains} records on the MCMC side, at least {need} needed (a 3 x 3 covariance of fewer samples '
                         f'is singular)')
    return out


class PosteriorComparison(_Recorder):
    """Two displacement covariance states, the VI side and the MCMC side, and the distances between the Gaussians they describe
    (posterior_comparison.py).  `record_vi(displacement)` takes the (C,3,D,H,W) float32 displacements of VI test samples,
    `record(displacement)` those of one recorded MCMC step, chains in order; `finalize` gives the four maps and the summary
    over a mask.  `records` counts the MCMC side, as the recorder loop reads it."""
    noun = 'posterior comparison'

    def __init__(self, dims, device):
        self.vi = DisplacementCovariance(dims, device)
        self.mcmc = DisplacementCovariance(dims, device)
        self.dims, self.device = self.mcmc.dims, device

    @property
    def records(self):
        return self.mcmc.records

    def record_vi(self, displacement):
        self.vi.record(displacement)

    def record(self, displacement):
        self.mcmc.record(displacement)

    def finalize(self, mask=None, scale=None, std_floor=1e-3):
        """-> ({'shift', 'log_std_ratio', 'bures', 'jeffreys'}: (D,H,W) float32 maps on the device, summary dict of
        posterior_comparison.comparison_summary).  scale: three positive floats, one per channel (default: voxel units);
        log_std_ratio < 0 where the VI posterior is the narrower.  One device-to-host read (the summary)."""
        for side, name in ((self.vi, 'VI'), (self.mcmc, 'MCMC')):
            if side.records < 2:
                raise RuntimeError(f'PosteriorComparison.finalize: {side.records} records on the {name} side, at least 2 needed')
        scale = self.mcmc.default_scale() if scale is None else tuple(float(s) for s in scale)
        *planes, isum, fsum = _pc.posterior_compare(self.vi.mean, self.vi.comoment, self.vi.records, self.mcmc.mean,
                                                    self.mcmc.comoment, self.mcmc.records, scale, std_floor,
                                                    _bool_mask(mask, self.device))
        return (dict(zip(_pc.COMPARISON_PLANES, planes)),
                _pc.comparison_summary(*_host_summary(isum, fsum), self.vi.records, self.mcmc.records))

    def state_dict(self):
        return {'vi': self.vi.state_dict(), 'mcmc': self.mcmc.state_dict()}

    def load_state_dict(self, sd):
        """both sides: the checkpoint's VI side replaces whatever this run's own VI stage recorded"""
        self.vi.load_state_dict(sd['vi'])
        self.mcmc.load_state_dict(sd['mcmc'])


QUANTILE_OPTION_KEYS = ('period', 'probs', 'bins', 'bin_width')
QUANTILE_METRICS = ('width_mean', 'width_max', 'width_x', 'width_y', 'width_z', 'out_of_range_frac', 'clipped_frac')
QUANTILE_MAX_RECORDS = 65535  # the uint16 counts (IRS_QUANTILE_MAX_RECORDS)
QUANTILE_DEFAULTS = {'probs': (0.05, 0.5, 0.95), 'bins': 64, 'bin_width': 0.125}


def _quantile_probs(probs, what):
    if isinstance(probs, (str, bytes)) or not hasattr(probs, '__len__'):
        raise ValueError(f'{what}: probs must be a list of probabilities, got {probs!r}')
    if any(isinstance(p, bool) or not isinstance(p, numbers.Real) for p in probs):
        raise ValueError(f'{what}: probs must be numbers, got {list(probs)!r}')
    probs = tuple(float(p) for p in probs)
    if not 2 <= len(probs) <= 8:
        raise ValueError(f'{what}: 2 to 8 probabilities, got {len(probs)}')
    if not all(0.0 < p < 1.0 for p in probs) or any(b <= a for a, b in zip(probs, probs[1:])):
        raise ValueError(f'{what}: probs must be strictly increasing in (0,1), got {list(probs)}')
    return probs


def _quantile_bins(bins, what):
    if isinstance(bins, bool) or not isinstance(bins, numbers.Integral):
        raise ValueError(f'{what}: bins must be an integer, got {bins!r}')
    if not 4 <= bins <= 256 or bins % 2:
        raise ValueError(f'{what}: bins must be an even number in 4..256, got {bins}')
    return int(bins)


def _quantile_bin_width(w, what):
    if isinstance(w, bool) or not isinstance(w, numbers.Real) or not (math.isfinite(w) and w > 0):
        raise ValueError(f'{what}: bin_width must be a finite number > 0, got {w!r}')
    return float(w)


def displacement_quantiles_options(cfg_trainer):
    """`trainer.displacement_quantiles` -> None when off, else {'period': P, 'probs': (...), 'bins': B, 'bin_width': w}.
    Absent / false / null: off.  true: P = log_period_MCMC, probs (0.05, 0.5, 0.95), 64 bins of 0.125 voxels.  A dict sets any
    of the four keys.  Refuses unknown keys, a non-integer P or P < 1, probs that are not 2 to 8 strictly increasing numbers in
    (0,1), bins that are not an even integer in 4..256, a bin_width that is not a finite number > 0, a config that records no
    step (no_samples_MCMC // P < 1) and one that would record more than 65535 displacements (a uint16 count)."""
    what = 'trainer.displacement_quantiles'

    def own_keys(opt):
        own = {**QUANTILE_DEFAULTS, **{k: v for k, v in opt.items() if k != 'period'}}
        return {'probs': _quantile_probs(own['probs'], what), 'bins': _quantile_bins(own['bins'], what),
                'bin_width': _quantile_bin_width(own['bin_width'], what)}

    return _record_options(cfg_trainer, 'displacement_quantiles', QUANTILE_OPTION_KEYS, f'a dict of {list(QUANTILE_OPTION_KEYS)}',
                           QUANTILE_MAX_RECORDS, 'a uint16 count holds at most {}: raise `period`', own_keys)


def quantiles_summary(isummary, fsummary, n):
    """the summary of DESIGN.md section 6 from the finalize's reduced columns (host ints / floats): isummary {voxels, voxels
    with an out-of-range quantile, samples in the two open-ended bins}, fsummary {sum / max of the band's width, sums of the
    per-channel widths} over the in-range masked voxels, n records.  The means are over the in-range masked voxels and NaN
    when there is none; out_of_range_frac = out-of-range voxels / voxels and clipped_frac = clipped samples / (3 n voxels)
    are NaN for an empty mask."""
    voxels, out_of_range, clipped = (int(x) for x in isummary)
    w_sum, w_max, wx, wy, wz = (float(x) for x in fsummary)
    inside = voxels - out_of_range
    nan = float('nan')
    return {'records': int(n), 'voxels': voxels, 'out_of_range_voxels': out_of_range, 'clipped_samples': clipped,
            'width_mean': _nan_div(w_sum, inside), 'width_max': w_max if inside else nan,
            'width_x': _nan_div(wx, inside), 'width_y': _nan_div(wy, inside), 'width_z': _nan_div(wz, inside),
            'out_of_range_frac': _nan_div(out_of_range, voxels), 'clipped_frac': _nan_div(clipped, 3 * int(n) * voxels)}


class DisplacementQuantiles(_Recorder):
    """Per voxel and channel, a histogram of the displacement over the recorded samples, pooled over chains, on the device:
    `centre` (3,D,H,W) float32, the displacement of the very first record, and `hist` (3,bins,D,H,W) uint16, bin-major (one
    bin of one channel is a contiguous volume).  That is 12 + 6 * bins bytes per voxel whatever the number of records: 396
    bytes per voxel at 64 bins, 6.6 GB at 256^3.  A count is a uint16, so at most 65535 records are taken.

    `bin_width` is in the units of `scale` (three positive floats, one per channel; default: voxels, as
    DisplacementCovariance.default_scale): channel a's bins are width_a = float32(bin_width / scale_a) wide in normalised
    coordinates, and inv_width_a = float32(1) / width_a, computed once, in float32, on the host.  Bins 0 and bins - 1 are
    open-ended; a quantile that falls into one of them is out of range and reported as NaN.
    `record(displacement)` takes the (C,3,D,H,W) float32 displacements of one step; `finalize(probs)` gives the quantile
    maps, the width of the band between the first and the last probability and the summary over a mask."""
    noun, max_records, exceed = 'displacement quantiles', QUANTILE_MAX_RECORDS, 'exceed the {} a uint16 count holds'

    def __init__(self, dims, device, bins=64, bin_width=0.125, scale=None):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 2:
            raise ValueError(f'displacement quantiles: three dims of at least 2, got {self.dims}')
        self.device = device
        self.bins = _quantile_bins(bins, 'displacement quantiles')
        self.bin_width = _quantile_bin_width(bin_width, 'displacement quantiles')
        scale = self.default_scale() if scale is None else tuple(float(s) for s in scale)
        if len(scale) != 3 or not all(math.isfinite(s) and s > 0 for s in scale):
            raise ValueError(f'displacement quantiles: scale must hold three finite floats > 0, got {scale}')
        self.scale = scale
        with np.errstate(all='ignore'):
            self.width = tuple(np.float32(self.bin_width / s) for s in scale)
            self.inv_width = tuple(np.float32(1) / w for w in self.width)
        if not all(np.isfinite(w) and w > 0 and np.isfinite(i) and i > 0 for w, i in zip(self.width, self.inv_width)):
            raise ValueError(f'displacement quantiles: bin_width {self.bin_width} over scale {scale} is not a float32 width')
        self.centre = torch.zeros((3,) + self.dims, device=device, dtype=torch.float32)
        self.hist = torch.zeros((3, self.bins) + self.dims, device=device, dtype=torch.int16).view(torch.uint16)

    @staticmethod
    def bytes_per_voxel(bins):
        return 12 + 6 * int(bins)

    def state_bytes(self):
        D, H, W = self.dims
        return self.bytes_per_voxel(self.bins) * D * H * W

    def default_scale(self):
        return voxel_scale(self.dims)

    def _update(self, displacement):
        ops.displacement_quantiles_update(displacement, self.centre, self.hist, self.inv_width, self.records)

    def histogram(self):
        """-> (3,bins,D,H,W) int32 on the device: the counts; every voxel and channel sums to `records`"""
        self._need_records('histogram')
        return self.hist.view(torch.int16).to(torch.int32) & 0xFFFF

    def finalize(self, probs, mask=None):
        """-> (quantiles (P,3,D,H,W), ci_width (D,H,W), float32 on the device, in the units of `scale`, NaN where out of
        range; summary dict of quantiles_summary).  One device-to-host read (the summary)."""
        self._need_records('finalize')
        probs = _quantile_probs(probs, 'displacement quantiles')
        quantiles, ci_width, isum, fsum = ops.displacement_quantiles_finalize(self.centre, self.hist, self.records, self.width,
                                                                              self.scale, probs, _bool_mask(mask, self.device))
        return quantiles, ci_width, quantiles_summary(*_host_summary(isum, fsum), self.records)

    def state_dict(self):
        return {'centre': self.centre.detach().cpu(), 'hist': self.hist.detach().cpu(), 'records': self.records,
                'bins': self.bins, 'bin_width': self.bin_width}

    def load_state_dict(self, sd):
        if int(sd['bins']) != self.bins or float(sd['bin_width']) != self.bin_width:
            raise ValueError(f'displacement quantiles with {sd["bins"]} bins of width {sd["bin_width"]} do not match this run '
                             f'({self.bins} bins of width {self.bin_width})')
        for key, lead, dtype in (('centre', (3,), torch.float32), ('hist', (3, self.bins), torch.uint16)):
            if tuple(sd[key].shape) != lead + self.dims or sd[key].dtype != dtype:
                raise ValueError(f'displacement quantiles of shape {tuple(sd[key].shape)} {sd[key].dtype} ({key}) do not match '
                                 f'this run ({lead + self.dims} {dtype})')
        records = int(sd['records'])
        if not 0 <= records <= QUANTILE_MAX_RECORDS:
            raise ValueError(f'displacement quantiles: {records} records, 0..{QUANTILE_MAX_RECORDS} expected')
        self.centre.copy_(sd['centre'])
        self.hist.view(torch.int16).copy_(sd['hist'].view(torch.int16))
        self.records = records


ICE_OPTION_KEYS = ('period', 'threshold', 'moving_space_dice')
ICE_DEFAULTS = {'threshold': 0.5, 'moving_space_dice': False}  # 0.5 voxels: where a nearest-neighbour label flips
ICE_SPACES = ('fixed', 'moving')


def inverse_consistency_options(cfg_trainer):
    """`trainer.inverse_consistency` -> None when off, else {'period': P, 'threshold': t, 'moving_space_dice': bool}.
    Absent / false / null: off.  true: P = log_period_MCMC, threshold 0.5 voxels, no moving-space Dice.  A dict sets any of
    the three keys.  Refuses unknown keys, a non-integer P or P < 1, a threshold that is not a finite number > 0, a non-bool
    moving_space_dice, a config that records no step (no_samples_MCMC // P < 1) and one that would record more than 2^31 - 1
    maps."""
    what = 'trainer.inverse_consistency'

    def own_keys(opt):
        own = {**ICE_DEFAULTS, **{k: v for k, v in opt.items() if k != 'period'}}
        t = own['threshold']
        if not _number(t) or not (math.isfinite(t) and t > 0):
            raise ValueError(f'{what}.threshold must be a finite number > 0 (voxels), got {t!r}')
        if not isinstance(own['moving_space_dice'], bool):
            raise ValueError(f'{what}.moving_space_dice must be true or false, got {own["moving_space_dice"]!r}')
        return {'threshold': float(t), 'moving_space_dice': own['moving_space_dice']}

    return _record_options(cfg_trainer, 'inverse_consistency', ICE_OPTION_KEYS,
                           '{"period": P, "threshold": t, "moving_space_dice": bool}', MAX_RECORDS,
                           'the record count holds at most {}', own_keys)


def ice_chain_summary(isummary, fsummary):
    """one chain's row of ops.inverse_consistency's summary (host ints / floats) -> {'voxels', 'nonfinite_voxels', 'mean',
    'rms', 'max'} over the finite masked voxels, NaN when there is none"""
    voxels, nonfinite = (int(x) for x in isummary)
    total, total_sq, mx = (float(x) for x in fsummary)
    finite = voxels - nonfinite
    return {'voxels': voxels, 'nonfinite_voxels': nonfinite, 'mean': _nan_div(total, finite),
            'rms': math.sqrt(total_sq / finite) if finite else float('nan'), 'max': mx if finite else float('nan')}


def ice_map_summary(isummary, fsummary, n, threshold):
    """the summary of DESIGN.md section 6 from ops.inverse_consistency_finalize's columns (host ints / floats): isummary
    {voxels, voxels with a non-finite mean, voxels with peak > threshold}, fsummary {sum / max of the mean map, max of the peak
    map}, n records.  'mean' is the mean of the mean map over its finite masked voxels, 'max' the largest peak;
    frac_above_<threshold> = voxels whose peak exceeds it / voxels.  NaN for an empty mask or when nothing is finite."""
    voxels, nonfinite, above = (int(x) for x in isummary)
    m_sum, m_max, p_max = (float(x) for x in fsummary)
    finite = voxels - nonfinite
    nan = float('nan')
    return {'records': int(n), 'voxels': voxels, 'nonfinite_voxels': nonfinite, 'mean': _nan_div(m_sum, finite),
            'mean_max': m_max if finite else nan, 'max': p_max if math.isfinite(p_max) else nan,
            f'above_{threshold:g}': above, f'frac_above_{threshold:g}': _nan_div(above, voxels)}


class InverseConsistency(_Recorder):
    """Per voxel, the Welford mean and the running maximum of the inverse-consistency error of the recorded samples, in voxels,
    for both orders of composition: `mean['fixed']` / `peak['fixed']` of |phi^-1 o phi - id| on the fixed grid and
    `mean['moving']` / `peak['moving']` of |phi o phi^-1 - id| on the moving grid, all (D,H,W) float32 on the device (16 D H W
    bytes whatever the number of records).  `record((v, transformation, displacement))` takes the dense velocity (voxel
    units), the forward transformation ([-1,1] coordinates) and the forward displacement (voxels) of one step, each
    (C,3,D,H,W) float32: it integrates -v, composes in both orders and folds the 2 C norm maps in.  `last` keeps the per-chain
    summaries of that step over `step_masks` (a dict of the two masks, or None) and `last_inverse` the inverse
    (transformation, displacement) of that step; `finalize` gives the summaries of the four maps."""
    noun = 'inverse consistency'

    def __init__(self, dims, device, no_steps=12, step_masks=None):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 2:
            raise ValueError(f'inverse consistency: three dims of at least 2, got {self.dims}')
        self.device, self.no_steps = device, int(no_steps)
        self.step_masks = {k: None if step_masks is None else _bool_mask(step_masks.get(k), device) for k in ICE_SPACES}
        self.mean = {k: torch.zeros(self.dims, device=device, dtype=torch.float32) for k in ICE_SPACES}
        self.peak = {k: torch.zeros(self.dims, device=device, dtype=torch.float32) for k in ICE_SPACES}
        self.last, self.last_inverse = None, None

    def record(self, sample):
        v, transformation, displacement = sample
        if not (tuple(v.shape) == tuple(transformation.shape) == tuple(displacement.shape)):
            raise ValueError(f'inverse consistency: velocity {tuple(v.shape)}, transformation {tuple(transformation.shape)} and '
                             f'displacement {tuple(displacement.shape)} differ in shape')
        C = v.shape[0]
        if self.records + C > self.max_records:
            raise ValueError(f'{self.noun}: {self.records} + {C} records {self.exceed.format(self.max_records)}')
        self._update(v, transformation, displacement)
        self.records += C

    def _update(self, v, transformation, displacement):
        t_inv, d_inv = ops.svf_exp_inverse(v.contiguous(), self.no_steps)
        self.last_inverse = (t_inv, d_inv)
        pairs = {'fixed': (transformation, displacement, d_inv), 'moving': (t_inv, d_inv, displacement)}
        step = {}
        for key in ICE_SPACES:
            norm, _, isum, fsum = ops.inverse_consistency(*pairs[key], mask=self.step_masks[key])
            ops.inverse_consistency_update(norm, self.mean[key], self.peak[key], self.records)
            step[key] = (isum, fsum)
        self.last = step

    def last_summaries(self):
        """-> {'fixed': [per-chain dict of ice_chain_summary], 'moving': [...]} of the last recorded step.  One device-to-host
        read."""
        self._need_records('last_summaries')
        (fi, ff), (mi, mf) = self.last['fixed'], self.last['moving']
        C = fi.shape[0]
        ints, floats = _host_summary(torch.cat([fi.reshape(-1), mi.reshape(-1)]), torch.cat([ff.reshape(-1), mf.reshape(-1)]))
        ni, nf = fi.shape[1], ff.shape[1]
        out = {}
        for s, key in enumerate(ICE_SPACES):
            out[key] = [ice_chain_summary(ints[(s * C + c) * ni:(s * C + c + 1) * ni], floats[(s * C + c) * nf:(s * C + c + 1) * nf])
                        for c in range(C)]
        return out

    def finalize(self, masks=None, threshold=0.5):
        """masks: {'fixed': mask, 'moving': mask} (either may be missing / None: the whole volume).  -> {'fixed': summary,
        'moving': summary} of ice_map_summary, the fixed-grid maps over the fixed mask and the moving-grid maps over the moving
        mask.  One device-to-host read."""
        self._need_records('finalize')
        masks = masks or {}
        res = [ops.inverse_consistency_finalize(self.mean[k], self.peak[k], threshold, _bool_mask(masks.get(k), self.device))
               for k in ICE_SPACES]
        ints, floats = _host_summary(torch.cat([r[0] for r in res]), torch.cat([r[1] for r in res]))
        ni, nf = res[0][0].numel(), res[0][1].numel()
        return {k: ice_map_summary(ints[s * ni:(s + 1) * ni], floats[s * nf:(s + 1) * nf], self.records, threshold)
                for s, k in enumerate(ICE_SPACES)}

    def state_dict(self):
        sd = {'records': self.records}
        for k in ICE_SPACES:
            sd[f'mean_{k}'], sd[f'peak_{k}'] = self.mean[k].detach().cpu(), self.peak[k].detach().cpu()
        return sd

    def load_state_dict(self, sd):
        for k in ICE_SPACES:
            for name in (f'mean_{k}', f'peak_{k}'):
                if tuple(sd[name].shape) != self.dims:
                    raise ValueError(f'inverse consistency of shape {tuple(sd[name].shape)} ({name}) does not match this run '
                                     f'({self.dims})')
        for k in ICE_SPACES:
            self.mean[k].copy_(sd[f'mean_{k}'])
            self.peak[k].copy_(sd[f'peak_{k}'])
        self.records = int(sd['records'])


LANDMARK_OPTION_KEYS = ('period', 'fixed', 'moving', 'index_base', 'coverage_levels', 'inverse', 'synthetic')
LANDMARK_DEFAULTS = {'index_base': 0, 'coverage_levels': (0.5, 0.95), 'inverse': False, 'synthetic': False}
LANDMARK_METRICS = ('of_mean_mean', 'of_mean_median', 'of_mean_max', 'sample_mean', 'sample_max')


def _coverage_levels(levels, what):
    if isinstance(levels, (str, bytes)) or not hasattr(levels, '__len__'):
        raise ValueError(f'{what}: coverage_levels must be a list of levels, got {levels!r}')
    if any(not _number(p) for p in levels):
        raise ValueError(f'{what}: coverage_levels must be numbers, got {list(levels)!r}')
    levels = tuple(float(p) for p in levels)
    if not 1 <= len(levels) <= 8:
        raise ValueError(f'{what}: 1 to 8 coverage levels, got {len(levels)}')
    if not all(0.0 < p < 1.0 for p in levels) or any(b <= a for a, b in zip(levels, levels[1:])):
        raise ValueError(f'{what}: coverage_levels must be strictly increasing in (0,1), got {list(levels)}')
    return levels


def landmark_options(cfg_trainer, data_loader=None):
    """`trainer.landmarks` -> None when off, else {'period': P, 'fixed': indices or None, 'moving': indices or None,
    'index_base': 0 | 1, 'coverage_levels': (...), 'inverse': bool, 'synthetic': bool}.
    Absent / false / null: off.  A dict: "fixed" and "moving" name two landmark files (landmarks.read_points: voxel indices of
    the native volumes, or of the registration grid for a loader without native volumes) with equal counts, read here into
    (K,3) arrays; "synthetic": true stands in for both when the loader is the synthetic one (`data_loader.native` None) and
    takes data_loader.synthetic_landmarks; "period" defaults to log_period_MCMC; "inverse": true also carries the moving
    landmarks into the fixed space.  Refuses `true` (the files must be named), unknown keys, a non-integer P or P < 1, an
    index_base other than 0 or 1, coverage_levels that are not 1 to 8 strictly increasing numbers in (0,1), a non-bool inverse
    or synthetic, paths given together with synthetic, a missing path or file, a malformed file, unequal counts, "synthetic"
    with a loader that reads files, a config that records no step and one that would record more than 2^31 - 1 samples."""
    from .landmarks import read_points
    what = 'trainer.landmarks'
    if cfg_trainer.get('landmarks') is True:
        raise ValueError(f'{what} must be false or a dict of {list(LANDMARK_OPTION_KEYS)} naming the two landmark files, got True')

    def own_keys(opt):
        own = {**LANDMARK_DEFAULTS, **{k: v for k, v in opt.items() if k != 'period'}}
        if isinstance(own['index_base'], bool) or own['index_base'] not in (0, 1):
            raise ValueError(f'{what}.index_base must be 0 or 1, got {own["index_base"]!r}')
        for key in ('inverse', 'synthetic'):
            if not isinstance(own[key], bool):
                raise ValueError(f'{what}.{key} must be true or false, got {own[key]!r}')
        out = {'index_base': int(own['index_base']), 'coverage_levels': _coverage_levels(own['coverage_levels'], what),
               'inverse': own['inverse'], 'synthetic': own['synthetic'], 'fixed': None, 'moving': None}
        if own['synthetic']:
            if 'fixed' in own or 'moving' in own:
                raise ValueError(f'{what}: "synthetic" stands in for the two files; "fixed" / "moving" must not be given with it')
            if data_loader is not None and getattr(data_loader, 'native', None) is not None:
                raise ValueError(f'{what}.synthetic: the data loader ({type(data_loader).__name__}) reads image files; its landmarks '
                                 f'come from "fixed" and "moving" files')
            return out
        for key in ('fixed', 'moving'):
            if not isinstance(own.get(key), str) or not own[key]:
                raise ValueError(f'{what}.{key}: the path of the {key} landmark file is required, got {own.get(key)!r}')
            try:
                out[key] = read_points(own[key], out['index_base'])
            except OSError as e:
                raise ValueError(f'{what}.{key}: cannot read {own[key]!r} ({e})') from e
        if len(out['fixed']) != len(out['moving']):
            raise ValueError(f'{what}: {len(out["fixed"])} fixed and {len(out["moving"])} moving landmarks; corresponding '
                             f'landmarks need equal counts')
        return out

    return _record_options(cfg_trainer, 'landmarks', LANDMARK_OPTION_KEYS, f'a dict of {list(LANDMARK_OPTION_KEYS)}', MAX_RECORDS,
                           'the record count holds at most {}', own_keys)


def landmark_metric_names(options, no_chains):
    """the metric names the option adds: the unregistered pair at step 0, every chain's record, the final summary"""
    names = [f'VI/train/TRE/{k}' for k in ('mean', 'median', 'max')]
    for d in ('TRE', 'TRE_inverse') if options['inverse'] else ('TRE',):
        names += [f'MCMC/chain_{i}/{d}/{k}' for i in range(no_chains) for k in ('mean', 'max')]
        names += [f'MCMC/{d}/{k}' for k in LANDMARK_METRICS] + [f'MCMC/{d}/coverage_{p:g}' for p in options['coverage_levels']]
        names.append(f'MCMC/{d}/error_spread_correlation')
    return names


class LandmarkPosterior(_Recorder):
    """The posterior of K landmarks carried through the sampled transformation, and of their target registration error, on the
    device in float64 (14 K numbers whatever the number of records).

    points / targets: (K,3) [-1,1] coordinates in x, y, z component order (landmarks.grid_points) of the landmarks in the space
    the displacement lives on and of the corresponding points in the space it maps to: fixed -> moving for the forward
    displacement, moving -> fixed for the one of ops.svf_exp_inverse.  scale: [-1,1] units -> the output unit per channel
    (default diagnostics.voxel_scale(dims): registration-grid voxels; NativeGrid.mm_scale() for mm); displacement_scale: what
    one [-1,1] unit is in the unit of the recorded displacement (default voxel_scale(dims): the trainer's displacements are
    in voxels; (1, 1, 1) for normalised ones).  `record(displacement)` takes the (C,3,D,H,W) float32 displacements of one
    step, chains in order; `last_tre()` the per-chain mean and max TRE of that step; `finalize(levels)` the table and the
    summary."""
    noun = 'landmark posterior'

    def __init__(self, points, targets, dims, device, scale=None, displacement_scale=None):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 2:
            raise ValueError(f'landmark posterior: three dims of at least 2, got {self.dims}')
        points, targets = (np.asarray(a, dtype=np.float64) for a in (points, targets))
        if points.ndim != 2 or points.shape[1] != 3 or points.shape != targets.shape or len(points) < 1:
            raise ValueError(f'landmark posterior: points and targets must both be (K,3) with K >= 1, got {points.shape} and '
                             f'{targets.shape}')
        if not (np.isfinite(points).all() and np.isfinite(targets).all()):
            raise ValueError('landmark posterior: the landmark coordinates must be finite')
        three = lambda name, v: self._three(name, voxel_scale(self.dims) if v is None else v)
        self.scale, self.displacement_scale = three('scale', scale), three('displacement_scale', displacement_scale)
        self.field_scale = tuple(s / d for s, d in zip(self.scale, self.displacement_scale))
        self.device, self.K = device, len(points)
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        sc = np.asarray(self.scale, dtype=np.float64)
        self.points, self.offset, self.target = to_dev(points), to_dev(points * sc), to_dev(targets * sc)
        self.state = ops.landmark_state(self.K, device)
        self.last_mapped = None

    @staticmethod
    def _three(name, values):
        values = tuple(float(v) for v in values)
        if len(values) != 3 or not all(math.isfinite(v) and v > 0 for v in values):
            raise ValueError(f'landmark posterior: {name} must hold three finite floats > 0, got {values}')
        return values

    def tre(self, mapped):
        """(C,K,3) mapped points on the device -> (C,K) float64 distances to the targets on the host (one copy)"""
        return (mapped.double() - self.target.double()).norm(dim=2).cpu()

    def initial_tre(self):
        """the TRE of the unregistered pair (zero displacement) per landmark, (K,) float64 on the host"""
        return (self.offset.double() - self.target.double()).norm(dim=1).cpu()

    def _update(self, displacement):
        self.last_mapped = ops.transform_points(self.points, displacement.contiguous(), self.field_scale, self.offset)
        ops.landmark_update(self.last_mapped, self.target, self.state, self.records)

    def last_tre(self):
        """-> (per-chain mean TRE, per-chain max TRE) of the record just taken over the landmarks with a finite mapped point,
        two lists of C floats (NaN when a chain has none).  One K-element device-to-host copy."""
        self._need_records('last_tre')
        e = self.tre(self.last_mapped).numpy()
        ok = np.isfinite(e)
        mean = [float(r[m].mean()) if m.any() else float('nan') for r, m in zip(e, ok)]
        peak = [float(r[m].max()) if m.any() else float('nan') for r, m in zip(e, ok)]
        return mean, peak

    def mean_points(self):
        """-> (K,3) float64 on the device: the posterior-mean mapped points, in the output unit"""
        self._need_records('mean_points')
        return self.state['mean']

    def finalize(self, levels=LANDMARK_DEFAULTS['coverage_levels']):
        """-> (table (K,10) float64 numpy with the columns ops.LANDMARK_COLUMNS, summary dict of landmarks.landmark_summary).
        One device-to-host read."""
        from .landmarks import landmark_summary
        self._need_records('finalize')
        levels = _coverage_levels(levels, 'landmark posterior')
        table, isum, fsum = ops.landmark_finalize(self.state, self.target)
        host = torch.cat([isum.view(torch.float64), fsum, table.reshape(-1)]).cpu()
        ni, nf = isum.numel(), fsum.numel()
        table_h = host[ni + nf:].reshape(table.shape).numpy()
        summary = landmark_summary(table_h, (host[:ni].view(torch.int64).tolist(), host[ni:ni + nf].tolist()), levels)
        summary['records'] = self.records
        return table_h, summary

    def state_dict(self):
        return {**{k: v.detach().cpu() for k, v in self.state.items()}, 'records': self.records,
                'points': self.points.detach().cpu(), 'target': self.target.detach().cpu()}

    def load_state_dict(self, sd):
        for key in ('points', 'target'):
            mine = getattr(self, key).detach().cpu()
            if tuple(sd[key].shape) != tuple(mine.shape) or not torch.equal(sd[key], mine):
                raise ValueError(f'landmark posterior: the {key} of the checkpoint ({tuple(sd[key].shape)}) are not those of this run '
                                 f'({tuple(mine.shape)})')
        for k, v in self.state.items():
            if tuple(sd[k].shape) != tuple(v.shape) or sd[k].dtype != v.dtype:
                raise ValueError(f'landmark posterior of shape {tuple(sd[k].shape)} {sd[k].dtype} ({k}) does not match this run '
                                 f'({tuple(v.shape)} {v.dtype})')
        for k, v in self.state.items():
            v.copy_(sd[k])
        self.records = int(sd['records'])


class LandmarkPair:
    """What `trainer.landmarks` records: `forward`, the fixed landmarks carried into the moving space by the sampled
    displacement, and with "inverse" also `inverse`, the moving landmarks carried into the fixed space by the displacement of
    exp(-v) (ops.svf_exp_inverse).  `record` takes the displacement, or (displacement, dense velocity) with an inverse."""

    def __init__(self, forward, inverse=None, no_steps=12):
        self.forward, self.inverse, self.no_steps = forward, inverse, int(no_steps)

    @property
    def records(self):
        return self.forward.records

    def directions(self):
        return [('TRE', self.forward)] + ([('TRE_inverse', self.inverse)] if self.inverse is not None else [])

    def record(self, sample):
        if self.inverse is None:
            self.forward.record(sample)
            return
        displacement, velocity = sample
        self.forward.record(displacement)
        self.inverse.record(ops.svf_exp_inverse(velocity.contiguous(), self.no_steps)[1])

    def state_dict(self):
        return {name: lp.state_dict() for name, lp in self.directions()}

    def load_state_dict(self, sd):
        if set(sd) != {name for name, _ in self.directions()}:
            raise ValueError(f'landmark posterior: the checkpoint holds {sorted(sd)}, this run records '
                             f'{[name for name, _ in self.directions()]} (trainer.landmarks.inverse differs)')
        for name, lp in self.directions():
            lp.load_state_dict(sd[name])


HAUSDORFF_MAX_PERCENTILES = 4  # IRS_HAUSDORFF_MAX_PERCENTILES


def hausdorff_options(cfg_trainer):
    """`trainer.hausdorff` -> None when off, else {'percentiles': (q, ...)}.
    Absent / false / null: off.  true: the percentiles (95,).  {"percentiles": [95, 99]}: those.  Refuses unknown keys and
    percentiles that are not 0 to 4 strictly increasing finite numbers in (0, 100]."""
    what = 'trainer.hausdorff'
    opt = cfg_trainer.get('hausdorff', False)
    if opt is None or opt is False:
        return None
    pct = (95.0,)
    if isinstance(opt, dict):
        unknown = set(opt) - {'percentiles'}
        if unknown:
            raise ValueError(f"{what}: unknown keys {sorted(unknown)}; known: ['percentiles']")
        if 'percentiles' in opt:
            pct = opt['percentiles']
            if not isinstance(pct, (list, tuple)) or len(pct) > HAUSDORFF_MAX_PERCENTILES:
                raise ValueError(f'{what}.percentiles must be a list of 0 to {HAUSDORFF_MAX_PERCENTILES} numbers, got {pct!r}')
            for q in pct:
                if not _number(q) or not math.isfinite(q) or not 0 < q <= 100:
                    raise ValueError(f'{what}.percentiles must lie in (0, 100], got {q!r}')
            if any(b <= a for a, b in zip(pct, pct[1:])):
                raise ValueError(f'{what}.percentiles must increase strictly, got {pct!r}')
            pct = tuple(float(q) for q in pct)
    elif opt is not True:
        raise ValueError(f'{what} must be true, false or {{"percentiles": [...]}}, got {opt!r}')
    return {'percentiles': pct}


def hausdorff_metric_names(options):
    """the metric names next to 'ASD' that the option adds: 'HD', then 'HD95' and the like"""
    return ['HD'] + [f'HD{q:g}' for q in options['percentiles']]


NATIVE_OPTION_KEYS = ('period', 'save')
NATIVE_SAVE_KEYS = ('im', 'seg', 'displacement')


def native_resolution_options(cfg_trainer, data_loader=None):
    """`trainer.native_resolution` -> None when off, else {'period': P or None, 'save': (...)}.
    Absent / false / null: off.  true: the native metrics at every logged step, the warped image of a saved sample.
    {"period": P, "save": [...]}: also at every P-th step after the burn-in; `save` lists what a saved sample writes on the
    native grid, a subset of "im", "seg", "displacement".  Refuses unknown keys, a non-integer P or P < 1, a `save` that is not
    a list of those names and -- when `data_loader` is given -- a loader without native volumes (`data_loader.native` None:
    the synthetic pair, which has no resolution but `dims`)."""
    what = 'trainer.native_resolution'
    opt = cfg_trainer.get('native_resolution', False)
    if opt is None or opt is False:
        return None
    period, save = None, ('im',)
    if isinstance(opt, dict):
        unknown = set(opt) - set(NATIVE_OPTION_KEYS)
        if unknown:
            raise ValueError(f'{what}: unknown keys {sorted(unknown)}; known: {list(NATIVE_OPTION_KEYS)}')
        if 'period' in opt:
            p = opt['period']
            if isinstance(p, bool) or not isinstance(p, numbers.Integral):
                raise ValueError(f'{what}.period must be an integer, got {p!r}')
            if p < 1:
                raise ValueError(f'{what}: the period must be >= 1, got {p}')
            period = int(p)
        if 'save' in opt:
            save = opt['save']
            if not isinstance(save, (list, tuple)) or any(s not in NATIVE_SAVE_KEYS for s in save) or len(set(save)) != len(save):
                raise ValueError(f'{what}.save must be a list of distinct names out of {list(NATIVE_SAVE_KEYS)}, got {save!r}')
            save = tuple(s for s in NATIVE_SAVE_KEYS if s in save)
    elif opt is not True:
        raise ValueError(f'{what} must be true, false or {{"period": P, "save": [...]}}, got {opt!r}')
    if data_loader is not None and getattr(data_loader, 'native', None) is None:
        raise ValueError(f'{what}: the data loader ({type(data_loader).__name__}) has no native volumes -- the synthetic pair exists '
                         f'at `dims` only; the option needs a BiobankDataLoader reading NIfTI files')
    return {'period': period, 'save': save}


SIMILARITY_OPTION_KEYS = ('bins', 'period')
SIMILARITY_METRICS = ('MSE', 'NCC', 'MI', 'NMI')  # the logged ones, in this order; ops.SIMILARITY_COLUMNS in lower case


def image_similarity_options(cfg_trainer):
    """`trainer.image_similarity` -> None when off, else {'bins': B, 'period': P or None}.
    Absent / false / null: off.  true: 64 bins, evaluated at every logged step.  {"bins": B, "period": P}: B bins per image
    (2 .. 128) and also at every P-th step after the burn-in.  Refuses unknown keys, a non-integer B or a B outside 2 .. 128, a
    non-integer P or P < 1."""
    what = 'trainer.image_similarity'
    opt = cfg_trainer.get('image_similarity', False)
    if opt is None or opt is False:
        return None
    bins, period = 64, None
    if isinstance(opt, dict):
        unknown = set(opt) - set(SIMILARITY_OPTION_KEYS)
        if unknown:
            raise ValueError(f'{what}: unknown keys {sorted(unknown)}; known: {list(SIMILARITY_OPTION_KEYS)}')
        if 'bins' in opt:
            b = opt['bins']
            if isinstance(b, bool) or not isinstance(b, numbers.Integral):
                raise ValueError(f'{what}.bins must be an integer, got {b!r}')
            if not 2 <= b <= 128:
                raise ValueError(f'{what}: bins must be in 2 .. 128, got {b}')
            bins = int(b)
        if 'period' in opt:
            p = opt['period']
            if isinstance(p, bool) or not isinstance(p, numbers.Integral):
                raise ValueError(f'{what}.period must be an integer, got {p!r}')
            if p < 1:
                raise ValueError(f'{what}: the period must be >= 1, got {p}')
            period = int(p)
    elif opt is not True:
        raise ValueError(f'{what} must be true, false or {{"bins": B, "period": P}}, got {opt!r}')
    return {'bins': bins, 'period': period}


def image_similarity_metric_names(no_chains):
    """the metric names the option adds: the unregistered pair at step 0, every chain's sampled transformation, the
    posterior-mean displacement"""
    prefixes = ['VI/train/similarity'] + [f'MCMC/chain_{i}/similarity' for i in range(no_chains)] + ['MCMC/similarity_of_mean']
    return [f'{p}/{k}' for p in prefixes for k in SIMILARITY_METRICS]


LOCAL_OPTION_KEYS = ('radius', 'period', 'save')
LOCAL_DEFAULTS = {'radius': 2, 'save': True}
LOCAL_MAX_RADIUS = 4  # IRS_LOCAL_MAX_RADIUS
LOCAL_METRICS = (('LNCC', 'lncc_mean'), ('LNCC_min', 'lncc_min'), ('SSIM', 'ssim_mean'))  # logged name, ops.LOCAL_COLUMNS name


def local_similarity_options(cfg_trainer):
    """`trainer.local_similarity` -> None when off, else {'period': P, 'radius': r, 'save': bool}.
    Absent / false / null: off.  true: windows of radius 2, the statistics at every logged step, the LNCC posterior recorded
    every log_period_MCMC-th step after the burn-in, the maps written.  {"radius": r, "period": P, "save": bool} sets any of
    them.  Refuses unknown keys, a non-integer r or an r outside 1 .. 4, a non-integer P or P < 1, a non-bool save, a config
    that records no step (no_samples_MCMC // P < 1) and one that would record more than 2^31 - 1 maps."""
    what = 'trainer.local_similarity'

    def own_keys(opt):
        own = {**LOCAL_DEFAULTS, **{k: v for k, v in opt.items() if k != 'period'}}
        r = own['radius']
        if isinstance(r, bool) or not isinstance(r, numbers.Integral):
            raise ValueError(f'{what}.radius must be an integer, got {r!r}')
        if not 1 <= r <= LOCAL_MAX_RADIUS:
            raise ValueError(f'{what}: radius must be in 1 .. {LOCAL_MAX_RADIUS}, got {r}')
        if not isinstance(own['save'], bool):
            raise ValueError(f'{what}.save must be true or false, got {own["save"]!r}')
        return {'radius': int(r), 'save': own['save']}

    return _record_options(cfg_trainer, 'local_similarity', LOCAL_OPTION_KEYS, '{"radius": r, "period": P, "save": bool}',
                           MAX_RECORDS, 'the sample count holds at most {}', own_keys)


def local_similarity_metric_names(no_chains):
    """the metric names the option adds: the unregistered pair at step 0, every chain's sampled transformation, the
    posterior-mean displacement"""
    prefixes = (['VI/train/local_similarity'] + [f'MCMC/chain_{i}/local_similarity' for i in range(no_chains)] +
                ['MCMC/local_similarity_of_mean'])
    return [f'{p}/{k}' for p in prefixes for k, _ in LOCAL_METRICS]


def local_map_summary(isummary, fsummary, n):
    """the summary of the LNCC posterior from ops.local_similarity_finalize's columns (host ints / floats): isummary {voxels,
    voxels without a defined sample}, fsummary {sum / min of the mean map, min of the minimum map} over the others, n records.
    'lncc_mean' is the mean of the mean map; NaN when no masked voxel has a sample."""
    voxels, empty = (int(x) for x in isummary)
    m_sum, m_min, l_min = (float(x) for x in fsummary)
    some = voxels - empty
    nan = float('nan')
    return {'records': int(n), 'voxels': voxels, 'empty_voxels': empty, 'lncc_mean': _nan_div(m_sum, some),
            'lncc_mean_min': m_min if some else nan, 'lncc_min': l_min if some else nan}


class LocalSimilarity(_Recorder):
    """Per voxel, the streaming mean, the minimum and the number of the LNCC samples that are defined there (a sample is NaN
    where its window is flat or holds a non-finite value, and is skipped): `mean`, `low` (D,H,W) float32 and `count` (D,H,W)
    int32 on the device, 12 D H W bytes whatever the number of records.  A low mean says every sample disagrees with the fixed
    image there; a high mean with a low minimum says the chain is unsure.  `record(lncc)` takes the (C,1,D,H,W) float32 LNCC
    maps of one step (ops.local_similarity); `finalize(mask)` gives the two maps, NaN where nothing was ever defined, and
    their summary over the mask."""
    noun = 'local similarity'

    def __init__(self, dims, device):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError(f'local similarity: three dims of at least 1, got {self.dims}')
        self.device = device
        self.mean = torch.zeros(self.dims, device=device, dtype=torch.float32)
        self.low = torch.full(self.dims, math.inf, device=device, dtype=torch.float32)
        self.count = torch.zeros(self.dims, device=device, dtype=torch.int32)

    def _update(self, lncc):
        ops.local_similarity_update(lncc.contiguous(), self.mean, self.low, self.count, self.records)

    def finalize(self, mask=None):
        """-> (mean, low (D,H,W) float32 with NaN where no sample was defined, summary of local_map_summary over the mask).  One
        device-to-host read."""
        self._need_records('finalize')
        isum, fsum = ops.local_similarity_finalize(self.mean, self.low, self.count, _bool_mask(mask, self.device))
        some = self.count > 0
        nan = self.mean.new_full((), math.nan)
        return self.mean.where(some, nan), self.low.where(some, nan), local_map_summary(*_host_summary(isum, fsum), self.records)

    def state_dict(self):
        return {'records': self.records, 'mean': self.mean.detach().cpu(), 'low': self.low.detach().cpu(),
                'count': self.count.detach().cpu()}

    def load_state_dict(self, sd):
        for name in ('mean', 'low', 'count'):
            if tuple(sd[name].shape) != self.dims:
                raise ValueError(f'local similarity state of shape {tuple(sd[name].shape)} ({name}) does not match this run '
                                 f'({self.dims})')
        self.mean.copy_(sd['mean'])
        self.low.copy_(sd['low'])
        self.count.copy_(sd['count'])
        self.records = int(sd['records'])


RESIDUAL_OPTION_KEYS = ('bins', 'range', 'period', 'nll_map', 'save')
RESIDUAL_DEFAULTS = {'bins': 128, 'range': None, 'nll_map': True, 'save': True}
RESIDUAL_MAX_BINS = 512  # IRS_RESIDUAL_MAX_BINS
# logged name -> how it follows from a row of residual_check.residual_fit; the ratios are empirical over model
RESIDUAL_METRICS = (('KL', lambda r: r['kl']), ('TV', lambda r: r['tv']), ('KS', lambda r: r['ks']), ('chi2', lambda r: r['chi2']),
                    ('tail', lambda r: r['tail']), ('std_ratio', lambda r: _nan_div(r['std'], r['std_model'])),
                    ('kurtosis_ratio', lambda r: _nan_div(r['kurtosis'], r['kurtosis_model'])))
RESIDUAL_MAP_METRICS = ('nll_mean', 'nll_max')


def residual_check_options(cfg_trainer):
    """`trainer.residual_check` -> None when off, else {'period': P, 'bins': B, 'range': h or None, 'nll_map': bool, 'save':
    bool}.  Absent / false / null: off.  true: 128 bins over +- the largest finite |z| of the unregistered pair's masked
    residual, the statistics at every logged step, the histogram and the NLL map recorded every log_period_MCMC-th step after
    the burn-in, the files written.  {"bins": B, "range": h, "period": P, "nll_map": bool, "save": bool} sets any of them.
    Refuses unknown keys, a non-integer B or a B outside 2 .. 512, an h that is no finite number > 0, a non-integer P or P < 1,
    a non-bool nll_map or save, a config that records no step (no_samples_MCMC // P < 1) and one that would record more than
    2^31 - 1 volumes."""
    what = 'trainer.residual_check'

    def own_keys(opt):
        own = {**RESIDUAL_DEFAULTS, **{k: v for k, v in opt.items() if k != 'period'}}
        b = own['bins']
        if isinstance(b, bool) or not isinstance(b, numbers.Integral):
            raise ValueError(f'{what}.bins must be an integer, got {b!r}')
        if not 2 <= b <= RESIDUAL_MAX_BINS:
            raise ValueError(f'{what}: bins must be in 2 .. {RESIDUAL_MAX_BINS}, got {b}')
        h = own['range']
        if h is not None and not (_number(h) and math.isfinite(h) and h > 0):
            raise ValueError(f'{what}.range must be a finite number > 0, got {h!r}')
        for key in ('nll_map', 'save'):
            if not isinstance(own[key], bool):
                raise ValueError(f'{what}.{key} must be true or false, got {own[key]!r}')
        return {'bins': int(b), 'range': None if h is None else float(h), 'nll_map': own['nll_map'], 'save': own['save']}

    return _record_options(cfg_trainer, 'residual_check', RESIDUAL_OPTION_KEYS,
                           '{"bins": B, "range": h, "period": P, "nll_map": bool, "save": bool}', MAX_RECORDS,
                           'the sample count holds at most {}', own_keys)


def residual_check_metric_names(options, no_chains, vi=False):
    """the metric names the option adds: the unregistered pair at step 0, the VI sample when VI runs, every chain's sample, the
    histogram pooled over chains and records, and the two figures of the NLL map"""
    prefixes = (['VI/train/residuals'] + (['VI/residuals'] if vi else []) + [f'MCMC/chain_{i}/residuals' for i in range(no_chains)] +
                ['MCMC/residuals'])
    return ([f'{p}/{k}' for p in prefixes for k, _ in RESIDUAL_METRICS] +
            ([f'MCMC/residuals/{k}' for k in RESIDUAL_MAP_METRICS] if options['nll_map'] else []))


def residual_metrics(row):
    """a row of residual_check.residual_fit -> {logged name: value} in the order of RESIDUAL_METRICS"""
    return {k: f(row) for k, f in RESIDUAL_METRICS}


def residual_map_summary(isummary, fsummary, n):
    """the summary of the NLL map from residual_check.residual_nll_finalize's columns (host ints / floats): isummary {voxels,
    voxels without a finite residual}, fsummary {sum / max of the mean map} over the others, n records; NaN when no masked
    voxel has a sample"""
    voxels, empty = (int(x) for x in isummary)
    m_sum, m_max = (float(x) for x in fsummary)
    some = voxels - empty
    return {'records': int(n), 'voxels': voxels, 'empty_voxels': empty, 'nll_mean': _nan_div(m_sum, some),
            'nll_max': m_max if some else float('nan')}


class ResidualCheck(_Recorder):
    """Does the likelihood describe the residuals it is applied to?  Over the recorded steps: per chain the exact int64 histogram
    of the residual z over `bins` equal bins of [-half_range, half_range] under the fixed mask, its counts and moment sums
    (residual_check.residual_histogram: `hist` (C,bins), `counts` (C,3) int64, `sums` (C,4) float64), and -- with `nll_map` --
    per voxel the streaming mean of -log p(z) under the mixture of that step and the number of finite residuals (`mean` (D,H,W)
    float32, `count` (D,H,W) int32; residual_check.residual_nll_update), 8 D H W bytes whatever the number of records.
    `set_mixture` gives the mixture the next record is scored under; `record(residuals)` takes the (C,1,D,H,W) float32
    residuals of one step; `finalize(std, proportions, mask)` sets the pooled histogram against a mixture and summarises the
    map."""
    noun = 'residual check'

    def __init__(self, dims, no_chains, device, half_range, bins=128, mask=None, nll_map=True):
        self.dims, self.no_chains, self.bins = tuple(int(d) for d in dims), int(no_chains), int(bins)
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError(f'residual check: three dims of at least 1, got {self.dims}')
        self.device, self.nll_map = device, bool(nll_map)
        self.half_range = float(torch.tensor(float(half_range), dtype=torch.float32))  # the value the kernel bins with
        if not (math.isfinite(self.half_range) and self.half_range > 0):
            raise ValueError(f'residual check: half_range = {half_range!r}, a finite value > 0 needed')
        self.mask = None if mask is None else _bool_mask(mask, device).reshape(1, 1, *self.dims).contiguous()
        self.hist = torch.zeros((self.no_chains, self.bins), device=device, dtype=torch.int64)
        self.counts = torch.zeros((self.no_chains, 3), device=device, dtype=torch.int64)
        self.sums = torch.zeros((self.no_chains, 4), device=device, dtype=torch.float64)
        self.sums[:, 3] = -math.inf
        self.mean = torch.zeros(self.dims if self.nll_map else (0, 0, 0), device=device, dtype=torch.float32)
        self.count = torch.zeros(self.dims if self.nll_map else (0, 0, 0), device=device, dtype=torch.int32)
        self.mixture = None

    def set_mixture(self, log_weight, inv_std):
        self.mixture = (list(log_weight), list(inv_std))

    def _update(self, residuals):
        if residuals.shape[0] != self.no_chains:
            raise ValueError(f'residual check: {residuals.shape[0]} chains recorded, the state holds {self.no_chains}')
        residuals = residuals.contiguous()
        _rc.residual_histogram(residuals, self.mask, self.half_range, self.bins, self.hist, self.counts, self.sums, self.records)
        if self.nll_map:
            if self.mixture is None:
                raise RuntimeError('ResidualCheck.record: set_mixture first')
            _rc.residual_nll_update(residuals, *self.mixture, self.mean, self.count, self.records)

    def pooled(self):
        """-> (hist (bins,), counts (3,) int64, sums (4,) float64) on the host, over chains and records"""
        hist, counts, sums = self.hist.cpu(), self.counts.cpu(), self.sums.cpu()
        return hist.sum(0).numpy(), counts.sum(0).numpy(), np.concatenate([sums[:, :3].sum(0).numpy(), [float(sums[:, 3].max())]])

    def finalize(self, std, proportions, mask=None):
        """-> (the NLL map (D,H,W) float32 with NaN where no residual was ever finite -- None without nll_map --, summary):
        {'records', 'half_range', 'bins', 'fit': residual_fit of the pooled histogram against (std, proportions), 'n_nonfinite',
        'n_clipped'[, 'nll': residual_map_summary over the mask]}"""
        self._need_records('finalize')
        hist, counts, sums = self.pooled()
        summary = {'records': self.records, 'half_range': self.half_range, 'bins': self.bins,
                   'fit': _rc.residual_fit(hist, counts, sums, self.half_range, std, proportions),
                   'n_nonfinite': int(counts[1]), 'n_clipped': int(counts[2])}
        if not self.nll_map:
            return None, summary
        isum, fsum = _rc.residual_nll_finalize(self.mean, self.count, _bool_mask(mask, self.device))
        summary['nll'] = residual_map_summary(*_host_summary(isum, fsum), self.records)
        return self.mean.where(self.count > 0, self.mean.new_full((), math.nan)), summary

    _STATE = ('hist', 'counts', 'sums', 'mean', 'count')

    def state_dict(self):
        return {'records': self.records, 'half_range': self.half_range, **{k: getattr(self, k).detach().cpu() for k in self._STATE}}

    def load_state_dict(self, sd):
        for name in self._STATE:
            if tuple(sd[name].shape) != tuple(getattr(self, name).shape):
                raise ValueError(f'residual check state of shape {tuple(sd[name].shape)} ({name}) does not match this run '
                                 f'({tuple(getattr(self, name).shape)})')
        for name in self._STATE:
            getattr(self, name).copy_(sd[name])
        self.half_range = float(sd['half_range'])
        self.records = int(sd['records'])


SURFACE_OPTION_KEYS = ('period', 'coverage', 'save')
SURFACE_DEFAULTS = {'coverage': (0.5, 0.9, 0.95), 'save': True}
SURFACE_MAX_LEVELS = 4  # IRS_SURFACE_MAX_LEVELS
SURFACE_METRICS = ('bias', 'abs_bias', 'std')  # logged per structure, before the coverage levels
SURFACE_COUNTS = ('contour_voxels', 'sampled_voxels', 'spread_voxels')  # ops.SURFACE_INT_COLUMNS


def _surface_coverage(levels, what):
    if isinstance(levels, (str, bytes)) or not hasattr(levels, '__len__'):
        raise ValueError(f'{what}: coverage must be a list of levels, got {levels!r}')
    if any(not _number(p) for p in levels):
        raise ValueError(f'{what}: coverage must be numbers, got {list(levels)!r}')
    levels = tuple(float(p) for p in levels)
    if len(levels) > SURFACE_MAX_LEVELS:
        raise ValueError(f'{what}: 0 to {SURFACE_MAX_LEVELS} coverage levels, got {len(levels)}')
    if not all(0.0 < p < 1.0 for p in levels) or any(b <= a for a, b in zip(levels, levels[1:])):
        raise ValueError(f'{what}: coverage must be strictly increasing in (0,1), got {list(levels)}')
    return levels


def surface_posterior_options(cfg_trainer):
    """`trainer.surface_posterior` -> None when off, else {'period': P, 'coverage': (...), 'save': bool}.
    Absent / false / null: off.  true: recorded every log_period_MCMC-th step after the burn-in, coverage at 0.5, 0.9 and 0.95,
    the maps written.  {"period": P, "coverage": [..], "save": bool} sets any of them.  Refuses unknown keys, a non-integer P or
    P < 1, a coverage that is not 0 to 4 strictly increasing numbers in (0,1), a non-bool save, a config that records no step
    (no_samples_MCMC // P < 1) and one that would record more than 2^31 - 1 samples."""
    what = 'trainer.surface_posterior'

    def own_keys(opt):
        own = {**SURFACE_DEFAULTS, **{k: v for k, v in opt.items() if k != 'period'}}
        if not isinstance(own['save'], bool):
            raise ValueError(f'{what}.save must be true or false, got {own["save"]!r}')
        return {'coverage': _surface_coverage(own['coverage'], what), 'save': own['save']}

    return _record_options(cfg_trainer, 'surface_posterior', SURFACE_OPTION_KEYS, '{"period": P, "coverage": [..], "save": bool}',
                           MAX_RECORDS, 'the sample count holds at most {}', own_keys)


def surface_coverage_key(level):
    """0.5 -> 'coverage_50', 0.95 -> 'coverage_95', 0.999 -> 'coverage_99.9'"""
    return f'coverage_{round(100.0 * level, 6):g}'


def surface_metric_names(options, structures):
    """the metric names the option adds, written at the end of the run"""
    keys = list(SURFACE_METRICS) + [surface_coverage_key(q) for q in options['coverage']]
    return [f'MCMC/surface/{k}/{s}' for k in keys for s in structures]


def surface_summary(isummary, fsummary, names, levels, n):
    """the per-structure summary of the surface posterior from ops.surface_posterior_finalize's columns (host rows of ints /
    floats, one per structure): -> {'records': n, 'structures': {name: {'bias' (mean signed distance), 'abs_bias', 'rms_bias',
    'max_abs_bias' over the contour voxels with a sample; 'std', 'max_std', 'coverage_XX' (the fraction whose normal band of
    that level holds the fixed boundary) over those with two; 'contour_voxels', 'sampled_voxels', 'spread_voxels'}}}.  NaN
    where the structure has no contour voxel with enough samples."""
    nan = float('nan')
    structures = {}
    for name, irow, frow in zip(names, isummary, fsummary):
        irow = [int(x) for x in irow]
        b_sum, ab_sum, b2_sum, ab_max, sd_sum, sd_max = (float(x) for x in frow)
        contour, some, two = irow[:3]
        st = {'bias': _nan_div(b_sum, some), 'abs_bias': _nan_div(ab_sum, some),
              'rms_bias': math.sqrt(b2_sum / some) if some else nan, 'max_abs_bias': ab_max if some else nan,
              'std': _nan_div(sd_sum, two), 'max_std': sd_max if two else nan}
        for q, inside in zip(levels, irow[3:]):
            st[surface_coverage_key(q)] = _nan_div(float(inside), two)
        st.update(contour_voxels=contour, sampled_voxels=some, spread_voxels=two)
        structures[name] = st
    return {'records': int(n), 'structures': structures}


class SurfacePosterior(_Recorder):
    """Per voxel of the fixed contour of every structure of `structures_dict`, the Welford moments of the signed distance to
    the same structure's contour in the recorded warps of the moving segmentation (ops.surface_posterior_update): `mean`, `m2`
    (D,H,W) float32 and `count` (D,H,W) int32 on the device, 12 D H W bytes whatever the number of records or structures (a
    voxel has one fixed label).  The mean is negative where the warped structure covers the fixed boundary (too large there),
    positive where it falls short; the spread says where on the boundary the chain is unsure, in the unit of `spacing`.
    `record(seg_warped)` takes the (C,1,D,H,W) int16 maps of one step, chains in order; `finalize(mask)` gives the two maps,
    NaN off the contours, and the summary per structure."""
    noun = 'surface posterior'

    def __init__(self, seg_fixed, structures_dict, spacing, device):
        self.names = list(structures_dict)
        self.labels = [int(structures_dict[k]) for k in self.names]
        if not 1 <= len(self.labels) <= 64:
            raise ValueError(f'surface posterior: 1 to 64 structures, got {len(self.labels)}')
        if len(set(self.labels)) != len(self.labels):
            raise ValueError(f'surface posterior: the label values {self.labels} are not distinct')
        self.spacing = tuple(float(x) for x in (spacing.tolist() if hasattr(spacing, 'tolist') else spacing))
        if len(self.spacing) != 3 or not all(math.isfinite(x) and x > 0.0 for x in self.spacing):
            raise ValueError(f'surface posterior: three finite spacings > 0, got {self.spacing}')
        if seg_fixed.dim() == 3:
            seg_fixed = seg_fixed[None, None]
        if seg_fixed.dim() != 5 or tuple(seg_fixed.shape[:2]) != (1, 1) or seg_fixed.dtype != torch.int16:
            raise ValueError(f'surface posterior: the fixed segmentation must be a (1,1,D,H,W) int16 volume, got '
                             f'{seg_fixed.dtype} {tuple(seg_fixed.shape)}')
        self.device = device
        self.seg_fixed = seg_fixed.to(device).contiguous()
        self.dims = tuple(int(d) for d in seg_fixed.shape[2:])
        self.mean = torch.zeros(self.dims, device=device, dtype=torch.float32)
        self.m2 = torch.zeros(self.dims, device=device, dtype=torch.float32)
        self.count = torch.zeros(self.dims, device=device, dtype=torch.int32)

    def _update(self, seg_warped):
        ops.surface_posterior_update(self.seg_fixed, seg_warped.contiguous(), self.labels, self.spacing, self.mean, self.m2,
                                     self.count)

    def finalize(self, mask=None, coverage=SURFACE_DEFAULTS['coverage']):
        """-> (bias, std (D,H,W) float32 on the device, NaN off the contours, summary dict of surface_summary over the mask).  One
        device-to-host read."""
        self._need_records('finalize')
        coverage = _surface_coverage(coverage, 'surface posterior')
        bias, std, isum, fsum = ops.surface_posterior_finalize(self.seg_fixed, self.labels, self.mean, self.m2, self.count,
                                                               coverage, _bool_mask(mask, self.device))
        ih, fh = _host_summary(isum.reshape(-1), fsum.reshape(-1))
        ni, nf = isum.shape[1], fsum.shape[1]
        rows = range(len(self.labels))
        summary = surface_summary([ih[j * ni:(j + 1) * ni] for j in rows], [fh[j * nf:(j + 1) * nf] for j in rows], self.names,
                                  coverage, self.records)
        return bias, std, summary

    def state_dict(self):
        return {'records': self.records, 'labels': list(self.labels), 'mean': self.mean.detach().cpu(), 'm2': self.m2.detach().cpu(),
                'count': self.count.detach().cpu()}

    def load_state_dict(self, sd):
        if [int(x) for x in sd['labels']] != self.labels:
            raise ValueError(f'surface posterior of labels {list(sd["labels"])} does not match this run ({self.labels})')
        for name in ('mean', 'm2', 'count'):
            if tuple(sd[name].shape) != self.dims:
                raise ValueError(f'surface posterior state of shape {tuple(sd[name].shape)} ({name}) does not match this run '
                                 f'({self.dims})')
        self.mean.copy_(sd['mean'])
        self.m2.copy_(sd['m2'])
        self.count.copy_(sd['count'])
        self.records = int(sd['records'])


NATIVE_POSTERIOR_OPTION_KEYS = ('period', 'labels', 'image', 'prob_maps', 'std_floor')
NATIVE_POSTERIOR_DEFAULTS = {'labels': True, 'image': True, 'prob_maps': False, 'std_floor': None}
NATIVE_POSTERIOR_IMAGE_METRICS = IMAGE_METRICS + IMAGE_Z_METRICS  # the native fixed image is always the reference


def native_posterior_options(cfg_trainer, data_loader=None):
    """`trainer.native_posterior` -> None when off, else {'period': P, 'labels': bool, 'image': bool, 'prob_maps': bool,
    'std_floor': float | None}.
    Absent / false / null: off.  true: both parts, recorded every log_period_MCMC-th step after the burn-in.  A dict sets any of
    "period", "labels", "image" (the two parts; at least one stays on), "prob_maps" (write the label probabilities) and
    "std_floor" (the floor of the z map: a number >= 0, or null for 1e-3 of the native moving image's intensity range).  Refuses
    unknown keys, a non-integer P or P < 1, a value of another type, both parts off, a config that records no step
    (no_samples_MCMC // P < 1) or more than 2^31 - 1 samples, the option without trainer.native_resolution (whose loader supplies
    the native pair) and -- when `data_loader` is given -- "labels" with a loader that found no segmentations."""
    what = 'trainer.native_posterior'

    def own_keys(opt):
        own = {**NATIVE_POSTERIOR_DEFAULTS, **{k: v for k, v in opt.items() if k != 'period'}}
        for key in ('labels', 'image', 'prob_maps'):
            if not isinstance(own[key], bool):
                raise ValueError(f'{what}.{key} must be true or false, got {own[key]!r}')
        if not own['labels'] and not own['image']:
            raise ValueError(f'{what}: "labels" and "image" are both false, nothing would be recorded')
        floor = own['std_floor']
        if floor is not None and (not _number(floor) or not math.isfinite(floor) or floor < 0):
            raise ValueError(f'{what}.std_floor must be a finite number >= 0 or null, got {floor!r}')
        own['std_floor'] = None if floor is None else float(floor)
        return own

    out = _record_options(cfg_trainer, 'native_posterior', NATIVE_POSTERIOR_OPTION_KEYS,
                          '{"period": P, "labels": bool, "image": bool, "prob_maps": bool, "std_floor": x}', MAX_RECORDS,
                          'the counts hold at most {}', own_keys)
    if out is None:
        return None
    if cfg_trainer.get('native_resolution', False) in (None, False):
        raise ValueError(f'{what} needs trainer.native_resolution, whose data loader supplies the pair on its own voxel grid')
    if out['labels'] and data_loader is not None and not getattr(data_loader, 'has_segs', True):
        raise ValueError(f'{what}: "labels" needs the fixed and the moving segmentation, and the data loader '
                         f'({type(data_loader).__name__}) found no "segs" directory')
    return out


def native_posterior_metric_names(options, structures):
    """the metric names the option adds: MCMC/native/seg/{metric}/{structure}, MCMC/native/seg/{entropy_mean,entropy_max,ECE} and
    MCMC/native/image/moving/{std_mean,std_max,range_max,z_rms,z_gt2,z_gt3}"""
    m = []
    if options['labels']:
        m += [f'MCMC/native/seg/{key}/{name}' for name in structures for key in LABEL_STRUCTURE_METRICS]
        m += [f'MCMC/native/seg/{key}' for key in ('entropy_mean', 'entropy_max', 'ECE')]
    if options['image']:
        m += [f'MCMC/native/image/moving/{key}' for key in NATIVE_POSTERIOR_IMAGE_METRICS]
    return m


class NativePosterior(_Recorder):
    """The label posterior and the image posterior on the image's own voxel grid (native_posterior.py): per native voxel the
    counts of every structure of `structures_dict` over the recorded nearest-neighbour warps of the native moving segmentation
    and / or the Welford mean / M2, minimum and maximum of the trilinear sample of the native moving image, on the device
    (4 K + 16 bytes per native voxel whatever the number of records).  `record(displacement)` takes the (C,3,*grid.dims)
    displacements of one step, chains in order, in voxels of the registration grid as the transition returns them (`voxels`
    False: in [-1,1] coordinates), in ONE launch; `finalize` gives the maps and the summaries.  moving_seg int16 / moving_im
    float32: (1,1,*grid.shape), each None when its part is off."""
    noun = 'native posterior'

    def __init__(self, grid, device, structures_dict=None, moving_seg=None, moving_im=None, fill=None, voxels=True):
        from . import native_posterior as _np_ops
        self._ops = _np_ops
        self.grid, self.device, self.voxels = grid, device, bool(voxels)
        self.names = list(structures_dict) if moving_seg is not None else []
        self.labels = [int(structures_dict[k]) for k in self.names]
        if moving_seg is None and moving_im is None:
            raise ValueError('native posterior: neither the moving segmentation nor the moving image is given')
        if moving_seg is not None and not 1 <= len(self.labels) <= 64:
            raise ValueError(f'native posterior: 1 to 64 structures, got {len(self.labels)}')
        if len(set(self.labels)) != len(self.labels):
            raise ValueError(f'native posterior: the label values {self.labels} are not distinct')
        if moving_im is not None and (fill is None or not math.isfinite(float(fill))):
            raise ValueError(f'native posterior: the moving image needs a finite fill, got {fill!r}')
        put = lambda t, dtype: None if t is None else t.to(device=device, dtype=dtype).contiguous()
        self.moving_seg, self.moving_im = put(moving_seg, torch.int16), put(moving_im, torch.float32)
        self.fill = 0.0 if fill is None else float(fill)
        self.state = _np_ops.native_posterior_state(grid, self.labels if moving_seg is not None else None, moving_im is not None,
                                                    device)

    @property
    def with_labels(self):
        return self.moving_seg is not None

    @property
    def with_image(self):
        return self.moving_im is not None

    def state_bytes(self):
        return self._ops.state_bytes(self.grid, len(self.labels), self.with_image)

    def _geometry(self):
        g = self.grid
        return [list(g.shape), list(g.padding), list(g.dims)]

    def _update(self, displacement):
        if self.voxels:
            from .utils.util import transform_coordinates
            displacement = transform_coordinates(displacement)
        self._ops.native_posterior_update(displacement.contiguous(), self.grid, self.state, self.records, seg=self.moving_seg,
                                          im=self.moving_im, fill=self.fill)

    def finalize(self, seg_fixed=None, im_fixed=None, mask=None, std_floor=0.0):
        """-> {'labels': {'entropy' float32, 'map' int16 (*grid.shape) on the device, 'summary': label_summary with the volumes
        in mm^3 under the header zooms}, 'image': {'mean', 'std', 'range'[, 'z'], 'summary': image_summary}}, each part when it
        is recorded.  seg_fixed: the NATIVE fixed segmentation (needed with the labels); im_fixed: the native fixed image, the
        reference of the z map, or None; mask: the native fixed mask or None.  One device-to-host read per part."""
        from . import _lib as L
        self._need_records('finalize')
        mask = _bool_mask(mask, self.device)
        out = {}
        if self.with_labels:
            if seg_fixed is None:
                raise ValueError('native posterior: finalize needs the native fixed segmentation')
            entropy, map_label, raw, ms = self._ops.native_label_finalize(self.state, self.records,
                                                                          seg_fixed.to(device=self.device, dtype=torch.int16), mask)
            host = torch.cat([raw.reshape(-1).view(torch.float64), ms, self.state['volume'].reshape(-1)]).cpu()
            KC = raw.numel()
            raw_h = host[:KC].view(torch.int64).reshape(raw.shape).numpy()
            ms_h, vol_h = host[KC:KC + 4].numpy(), host[KC + 4:].reshape(-1, 2).numpy()
            if ms_h[3] != 0:
                raise L.IrsError(f'native posterior: {int(ms_h[3])} voxels hold more than the {self.records} records counted: '
                                 f'the counts and the record number disagree')
            summary = label_summary(raw_h, vol_h, self.records, ms_h, self.names, self.grid.spacing_xyz())
            summary['raw'] = raw_h
            out['labels'] = {'entropy': entropy, 'map': map_label, 'summary': summary}
        if self.with_image:
            ref = None if im_fixed is None else im_fixed.to(device=self.device, dtype=torch.float32)
            std, rng, z, isum, fsum = self._ops.native_image_finalize(self.state, self.records, ref, std_floor, mask)
            mean = self.state['mean']
            out['image'] = {'mean': mean.where(mean.isfinite(), std.new_full((), math.nan)), 'std': std, 'range': rng,
                            'summary': image_summary(*_host_summary(isum, fsum), self.records, ref is not None)}
            if z is not None:
                out['image']['z'] = z
        return out

    def probabilities(self):
        """-> (K,*grid.shape) float32 on the device: counts / n"""
        self._need_records('probabilities')
        if not self.with_labels:
            raise RuntimeError('NativePosterior.probabilities: the labels are not recorded')
        return self.state['counts'].float() / self.records

    def state_dict(self):
        return {'records': self.records, 'labels': list(self.labels), 'geometry': self._geometry(), 'image': self.with_image,
                **{key: t.detach().cpu() for key, t in self.state.items() if key != 'labels'}}

    def load_state_dict(self, sd):
        if [int(x) for x in sd['labels']] != self.labels:
            raise ValueError(f'native posterior of labels {list(sd["labels"])} does not match this run ({self.labels})')
        if [list(int(x) for x in g) for g in sd['geometry']] != self._geometry():
            raise ValueError(f'native posterior of geometry {sd["geometry"]} (shape, padding, dims) does not match this run '
                             f'({self._geometry()})')
        if bool(sd['image']) != self.with_image:
            raise ValueError(f'native posterior {"with" if sd["image"] else "without"} the image part does not match this run')
        tensors = {key: t for key, t in self.state.items() if key != 'labels'}
        for key, t in tensors.items():
            if key not in sd or tuple(sd[key].shape) != tuple(t.shape):
                raise ValueError(f'native posterior state {key!r} of shape {tuple(sd[key].shape) if key in sd else None} does not '
                                 f'match this run ({tuple(t.shape)})')
        for key, t in tensors.items():
            t.copy_(sd[key])
        self.records = int(sd['records'])
