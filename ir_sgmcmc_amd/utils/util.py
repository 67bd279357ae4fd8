"""Numerics helpers with the reference's names (utils/util.py), backed by the HIP operators where there is volume work.

Tiny scalar / bookkeeping helpers (json io, MetricTracker, coordinate scaling of a whole tensor by a constant) are
plain host code, as in the reference.
"""
import json
import math
from collections import OrderedDict
from pathlib import Path

import torch

from .. import ops as _ops


def ensure_dir(dirname):
    dirname = Path(dirname)
    if not dirname.is_dir():
        dirname.mkdir(parents=True, exist_ok=False)


def read_json(fname):
    with Path(fname).open('rt') as handle:
        return json.load(handle, object_hook=OrderedDict)


def write_json(content, fname):
    with Path(fname).open('wt') as handle:
        json.dump(content, handle, indent=4, sort_keys=False)


def get_control_grid_size(dims, cps):
    """utils/util.py:61-69"""
    return _ops.control_grid_size(dims, cps)


def _axis_scale(field, inverse=False):
    # channel c <-> its own axis (x <-> W ...); identical to utils/util.py:418-443 for the cubic volumes it supports
    n = [float(s - 1) for s in reversed(field.shape[2:])]
    f = [(x / 2.0) if inverse else (2.0 / x) for x in n]
    return torch.tensor(f, dtype=field.dtype, device=field.device).view(1, -1, *([1] * (field.dim() - 2)))


def transform_coordinates(field):
    """absolute voxel units -> normalised [-1, 1] units (utils/util.py:418-429)"""
    return field * _axis_scale(field)


def transform_coordinates_inv(field):
    """normalised -> absolute voxel units (utils/util.py:432-443)"""
    return field * _axis_scale(field, inverse=True)


def init_identity_grid_3D(dims, device=None):
    """(1, D, H, W, 3) identity grid in [-1, 1], channel 0 = x = last axis (utils/util.py:263-278)"""
    nz, ny, nx = dims[0], dims[1], dims[2]
    x = torch.linspace(-1, 1, steps=nx, device=device).view(1, 1, nx).expand(nz, ny, nx)
    y = torch.linspace(-1, 1, steps=ny, device=device).view(1, ny, 1).expand(nz, ny, nx)
    z = torch.linspace(-1, 1, steps=nz, device=device).view(nz, 1, 1).expand(nz, ny, nx)
    return torch.stack((x, y, z), dim=-1).unsqueeze(0)


def get_noise_uniform(shape, device, alpha):
    return -2.0 * alpha * torch.rand(shape, device=device) + alpha


def get_noise_Langevin(sigma, tau):
    return math.sqrt(2.0 * tau) * sigma * torch.randn_like(sigma)


def add_noise_uniform_field(field, alpha):
    """utils/util.py:44-45"""
    return field + transform_coordinates(get_noise_uniform(field.shape, field.device, alpha))


def add_noise_Langevin(field, sigma, tau):
    """utils/util.py:48-49; eps is drawn with torch's device generator, the add runs in the HIP kernel"""
    return _ops.perturb_smooth(field.contiguous(), None, sigma.contiguous(), torch.randn_like(sigma), tau=tau)


def separable_conv_3D(field, *args):
    """Both branches of utils/util.py:350-406: (kernel (3,1,k), padding_sz) or (S_x, S_y, S_z, padding).

    The 2-argument branch (utils/util.py:362-392) pads the last axis by replicate, flattens the volume, runs a zero-padded
    conv1d and crops -- three times, permuting the axes in between.  The crop removes exactly the positions the zero padding
    and the neighbouring rows reach, so it IS one (2 p + 1)-tap filter per axis with replicate padding, like the 4-argument
    branch (verified against the imported reference to 3e-7 and pinned by tests/golden/utils_ops.npz, including per-channel
    kernels: `groups=3` gives channel c row c of the kernel tensor)."""
    k = args[0].reshape(args[0].shape[0], -1).detach().cpu()
    if len(args) == 4:  # the three axis kernels of every reference call site are the same taps reshaped
        ky, kz = (a.reshape(a.shape[0], -1).detach().cpu() for a in args[1:3])
        if not (torch.equal(k, ky) and torch.equal(k, kz)):
            raise NotImplementedError('separable_conv_3D: different kernels per axis')
    f = field.contiguous()
    if all(torch.equal(k[0], k[c]) for c in range(1, k.shape[0])):
        return _ops.perturb_smooth(f, k[0].tolist())
    out = torch.empty_like(f)
    for c in range(k.shape[0]):  # a kernel of its own per channel: filter with each, keep the matching channel
        out[:, c] = _ops.perturb_smooth(f, k[c].tolist())[:, c]
    return out


def calc_norm(field):
    """voxel-wise L2 norm of a batch of 3-D vector fields (utils/util.py:215-225)"""
    return torch.linalg.vector_norm(field, ord=2, dim=1, keepdim=True)


def calc_det_J(nabla):
    """utils/util.py:72-91 on an explicit nabla tensor (C,3,D,H,W,3)"""
    a, b, c = nabla[..., 0], nabla[..., 1], nabla[..., 2]
    return (a[:, 0] * b[:, 1] * c[:, 2] + b[:, 0] * c[:, 1] * a[:, 2] + c[:, 0] * a[:, 1] * b[:, 2]
            - a[:, 2] * b[:, 1] * c[:, 0] - b[:, 2] * c[:, 1] * a[:, 0] - c[:, 2] * a[:, 1] * b[:, 0])


def calc_no_non_diffeomorphic_voxels(transformation, diff_op=None):
    """(NaN count of log det J per chain as numpy, log det J) -- utils/util.py:209-212, one fused HIP kernel"""
    cnt, log_det = _ops.log_det_jacobian(transformation.contiguous())
    return cnt.cpu().numpy(), log_det


@torch.no_grad()
def calc_posterior_statistics(samples, device='cuda:0'):
    samples = samples.to(device)
    return torch.mean(samples, dim=0), torch.std(samples, dim=0)


@torch.no_grad()
def calc_split_rhat(samples, mask=None, thresholds=(1.01, 1.1)):
    """split-R-hat of the displacement samples (absent in the reference): samples (C, N, 3, D, H, W) on the device, every
    chain's N samples in order; mask (D,H,W) or None.  -> (map (D,H,W), summary dict), as diagnostics.ChainMoments.rhat."""
    from ..diagnostics import ChainMoments
    if samples.dim() != 6 or samples.shape[2] != 3:
        raise ValueError(f'samples must have shape (C, N, 3, D, H, W), got {tuple(samples.shape)}')
    C, N = samples.shape[:2]
    cm = ChainMoments(C, samples.shape[3:], N, samples.device)
    for i in range(N):
        cm.record(samples[:, i].float().contiguous())
    return cm.rhat(mask, thresholds)


@torch.no_grad()
def calc_split_ess(samples, mask=None, max_lag=32, threshold=400.0):
    """split ESS and MCSE of the displacement samples (absent in the reference): samples (C, N, 3, D, H, W) on the device,
    every chain's N samples in order; mask (D,H,W) or None.  -> (ESS map, MCSE map, summary dict), as
    diagnostics.ChainMoments.ess."""
    from ..diagnostics import ChainMoments
    if samples.dim() != 6 or samples.shape[2] != 3:
        raise ValueError(f'samples must have shape (C, N, 3, D, H, W), got {tuple(samples.shape)}')
    C, N = samples.shape[:2]
    cm = ChainMoments(C, samples.shape[3:], N, samples.device, max_lag=max_lag)
    for i in range(N):
        cm.record(samples[:, i].float().contiguous())
    return cm.ess(mask, threshold)


@torch.no_grad()
def calc_label_posterior(seg_samples, seg_fixed, structures_dict, spacing, mask=None):
    """posterior label maps of segmentation samples (absent in the reference): seg_samples (C, N, 1, D, H, W) int16 on the
    device, every chain's N warped maps in order (recorded step by step, chains in order within a step); seg_fixed (D,H,W)
    int16; mask (D,H,W) or None.  -> (entropy, map_label, summary dict), as diagnostics.LabelPosterior.finalize."""
    from ..diagnostics import LabelPosterior
    if seg_samples.dim() != 6 or seg_samples.shape[2] != 1:
        raise ValueError(f'seg_samples must have shape (C, N, 1, D, H, W), got {tuple(seg_samples.shape)}')
    C, N = seg_samples.shape[:2]
    lp = LabelPosterior(structures_dict, seg_samples.shape[3:], seg_samples.device)
    for i in range(N):
        lp.record(seg_samples[:, i].contiguous())
    return lp.finalize(seg_fixed, mask, spacing)


@torch.no_grad()
def calc_surface_posterior(seg_fixed, seg_samples, structures_dict, spacing, mask=None, coverage=(0.5, 0.9, 0.95)):
    """surface posterior of segmentation samples (absent in the reference): seg_fixed (D,H,W) or (1,1,D,H,W) int16; seg_samples
    (C, N, 1, D, H, W) int16 on the device, every chain's N warped maps in order (recorded step by step, chains in order within
    a step); spacing (sx, sy, sz); mask (D,H,W) or None; coverage: 0 to 4 increasing levels in (0,1).  -> (bias, std (D,H,W)
    float32 with NaN off the fixed contours, summary dict), as diagnostics.SurfacePosterior.finalize."""
    from ..diagnostics import SurfacePosterior
    if seg_samples.dim() != 6 or seg_samples.shape[2] != 1:
        raise ValueError(f'seg_samples must have shape (C, N, 1, D, H, W), got {tuple(seg_samples.shape)}')
    sp = SurfacePosterior(seg_fixed, structures_dict, spacing, seg_samples.device)
    for i in range(seg_samples.shape[1]):
        sp.record(seg_samples[:, i].contiguous())
    return sp.finalize(mask, coverage)


@torch.no_grad()
def calc_jacobian_posterior(transformations, mask=None):
    """Jacobian posterior maps of transformation samples (absent in the reference): transformations (n,3,D,H,W) float32 on the
    device, in normalised coordinates, the n records in order; mask (D,H,W) or None.  -> (fold_prob, logJ_mean, logJ_std,
    summary dict), as diagnostics.JacobianPosterior.finalize."""
    from .. import _lib as L
    from ..diagnostics import JacobianPosterior
    if transformations.dim() != 5 or transformations.shape[1] != 3:
        raise ValueError(f'transformations must have shape (n, 3, D, H, W), got {tuple(transformations.shape)}')
    jp = JacobianPosterior(transformations.shape[2:], transformations.device)
    for i in range(0, transformations.shape[0], L.IRS_MAX_CHAINS):  # one launch folds up to IRS_MAX_CHAINS records, in order
        jp.record(transformations[i:i + L.IRS_MAX_CHAINS].float().contiguous())
    return jp.finalize(mask)


@torch.no_grad()
def calc_structure_report(displacements, transformations, seg_fixed, structures_dict, spacing, mask=None, maps=None, chains=1):
    """Per-structure motion posterior of samples (absent in the reference): displacements (n,3,D,H,W) float32 in voxels and
    transformations (n,3,D,H,W) float32 in normalised coordinates on the device, the n records ordered by step, then by chain
    (`chains` per step); seg_fixed (D,H,W) int16; structures_dict {name: label}; spacing (sx, sy, sz); mask (D,H,W) or None;
    maps: {name: (D,H,W) float32 map} or None, whose per-structure rows are added.  -> the dict of
    structure_report.structure_summary with 'maps': the names of the maps, as Trainer.structure_summary; 'series': the (ints,
    floats) arrays behind it."""
    from .. import structure_report as sr
    from ..diagnostics import StructureReport
    for name, t in (('displacements', displacements), ('transformations', transformations)):
        if t.dim() != 5 or t.shape[1] != 3:
            raise ValueError(f'{name} must have shape (n, 3, D, H, W), got {tuple(t.shape)}')
    n = displacements.shape[0]
    report = StructureReport(seg_fixed, structures_dict, max(n, 1), displacements.device, mask=mask)
    for i in range(0, n, chains):  # one launch reduces the records of one step, in order
        report.record((displacements[i:i + chains].float().contiguous(), transformations[i:i + chains].float().contiguous()))
    summary, series = report.finalize([float(s) for s in spacing], chains)
    summary['maps'] = list(maps or {})
    if maps:
        stacked = torch.stack([m.to(displacements.device, torch.float32).reshape(report.dims) for m in maps.values()])
        sr.add_map_rows(summary, sr.structure_map_rows(*report.map_stats(stacked), summary['maps'], report.names), summary['maps'])
    summary['series'] = series
    return summary


@torch.no_grad()
def calc_truth_calibration(displacements, truth, mask=None, chains=1, scale=(1.0, 1.0, 1.0), levels=(0.5, 0.9, 0.95), pit_bins=20,
                           rank_bins=16, reliability_bins=16, std_floor=1e-3, reference='hotelling'):
    """Samples against a known displacement (absent in the reference): displacements (n,3,D,H,W) float32 on the device, n <= 65535
    records ordered by step, then by chain (`chains` per step); truth (3,D,H,W) float32 in the same unit; mask (D,H,W) or None;
    scale: three floats, one per channel, the unit of the errors.  -> (maps {'error', 'mahalanobis'}: (D,H,W) float32 on the
    device, summary dict of truth.calibration_summary with 'initial_*' the error of a zero displacement, series (ints (n,2),
    floats (n,3)) of the per-record error rows), as Trainer.truth_summary."""
    from ..diagnostics import TruthCalibration
    if displacements.dim() != 5 or displacements.shape[1] != 3:
        raise ValueError(f'displacements must have shape (n, 3, D, H, W), got {tuple(displacements.shape)}')
    n = displacements.shape[0]
    tc = TruthCalibration(truth, max(n, 1), displacements.device, scale, mask)
    for i in range(0, n, chains):  # one launch takes the records of one step, in order
        tc.record(displacements[i:i + chains].float().contiguous())
    return tc.finalize(None, levels, pit_bins, rank_bins, reliability_bins, std_floor, reference, initial=tc.initial_error())


@torch.no_grad()
def calc_image_posterior(volumes, transformations, reference=None, mask=None, std_floor=0.0):
    """Volumes carried through transformation samples (absent in the reference): volumes (S,1,D,H,W) float32 on the device, on
    the grid the transformations sample, S in 1 .. 8; transformations (n,3,D,H,W) float32 in normalised coordinates, the n
    records in order; reference: {index of a volume: (D,H,W) volume it is compared with} or None; mask (D,H,W) or None.
    -> one dict per volume {'mean', 'std', 'range'[, 'z'], 'summary'}, as diagnostics.ImagePosterior.finalize."""
    from .. import _lib as L
    from ..diagnostics import ImagePosterior
    if transformations.dim() != 5 or transformations.shape[1] != 3:
        raise ValueError(f'transformations must have shape (n, 3, D, H, W), got {tuple(transformations.shape)}')
    if volumes.dim() != 5 or volumes.shape[1] != 1 or volumes.shape[2:] != transformations.shape[2:]:
        raise ValueError(f'volumes must have shape (S, 1, {", ".join(str(n) for n in transformations.shape[2:])}), got '
                         f'{tuple(volumes.shape)}')
    names = [str(i) for i in range(volumes.shape[0])]
    ip = ImagePosterior(volumes, names, transformations.device)
    for i in range(0, transformations.shape[0], L.IRS_MAX_CHAINS):  # one launch folds up to IRS_MAX_CHAINS records, in order
        ip.record(transformations[i:i + L.IRS_MAX_CHAINS].float().contiguous())
    out = ip.finalize(mask, {str(k): v for k, v in (reference or {}).items()}, std_floor)
    return [out[name] for name in names]


@torch.no_grad()
def calc_displacement_covariance(displacements, mask=None, scale=None):
    """Principal spread and direction of displacement samples (absent in the reference): displacements (n,3,D,H,W) float32 on
    the device, in normalised coordinates, the n records in order; mask (D,H,W) or None; scale: three floats, one per channel
    (default: voxel units).  -> (std, direction, anisotropy, summary dict), as diagnostics.DisplacementCovariance.finalize."""
    from .. import _lib as L
    from ..diagnostics import DisplacementCovariance
    if displacements.dim() != 5 or displacements.shape[1] != 3:
        raise ValueError(f'displacements must have shape (n, 3, D, H, W), got {tuple(displacements.shape)}')
    dc = DisplacementCovariance(displacements.shape[2:], displacements.device)
    for i in range(0, displacements.shape[0], L.IRS_MAX_CHAINS):  # one launch folds up to IRS_MAX_CHAINS records, in order
        dc.record(displacements[i:i + L.IRS_MAX_CHAINS].float().contiguous())
    return dc.finalize(mask, scale)


@torch.no_grad()
def calc_displacement_modes(displacements, mask=None, modes=8, scale=None, chains=1):
    """Principal modes of displacement samples by the snapshot method (absent in the reference): displacements (n,3,D,H,W)
    float32 on the device, in normalised coordinates, 2 <= n <= 1024 records ordered by step, then by chain (`chains` per step);
    mask (D,H,W) or None: the voxels of the inner product; modes: 1 .. 16; scale: three floats, one per channel (default: voxel
    units).  -> the dict of diagnostics.DisplacementModes.finalize."""
    from ..diagnostics import DisplacementModes
    if displacements.dim() != 5 or displacements.shape[1] != 3:
        raise ValueError(f'displacements must have shape (n, 3, D, H, W), got {tuple(displacements.shape)}')
    dm = DisplacementModes(displacements.shape[2:], displacements.device, displacements.shape[0], mask)
    for i in range(0, displacements.shape[0], chains):  # one launch folds the records of one step, in order
        dm.record(displacements[i:i + chains].float().contiguous())
    return dm.finalize(modes, scale)


@torch.no_grad()
def calc_posterior_comparison(displacements_a, displacements_b, mask=None, scale=None, std_floor=1e-3):
    """The distances between the Gaussians fitted, per voxel, to two sets of displacement samples (absent in the reference):
    displacements_a (n_a,3,D,H,W) and displacements_b (n_b,3,D,H,W) float32 on the device, in normalised coordinates, at least
    2 records each; mask (D,H,W) or None; scale: three floats, one per channel (default: voxel units); std_floor: the floor of
    the Jeffreys divergence's eigenvalues, in the units of the scale.  -> ({'shift', 'log_std_ratio', 'bures', 'jeffreys'}: maps,
    summary dict), as diagnostics.PosteriorComparison.finalize with A in the role of the VI side."""
    from .. import _lib as L
    from ..diagnostics import PosteriorComparison
    for name, d in (('displacements_a', displacements_a), ('displacements_b', displacements_b)):
        if d.dim() != 5 or d.shape[1] != 3:
            raise ValueError(f'{name} must have shape (n, 3, D, H, W), got {tuple(d.shape)}')
    if tuple(displacements_a.shape[2:]) != tuple(displacements_b.shape[2:]):
        raise ValueError(f'the two sets of displacements live on different grids: {tuple(displacements_a.shape[2:])} and '
                         f'{tuple(displacements_b.shape[2:])}')
    pc = PosteriorComparison(displacements_a.shape[2:], displacements_a.device)
    for take, d in ((pc.record_vi, displacements_a), (pc.record, displacements_b)):
        for i in range(0, d.shape[0], L.IRS_MAX_CHAINS):  # one launch folds up to IRS_MAX_CHAINS records, in order
            take(d[i:i + L.IRS_MAX_CHAINS].float().contiguous())
    return pc.finalize(mask, scale, std_floor)


@torch.no_grad()
def calc_displacement_quantiles(displacements, probs=(0.05, 0.5, 0.95), mask=None, bins=64, bin_width=0.125, scale=None):
    """Per-voxel quantiles of displacement samples and the width of the band between the first and the last (absent in the
    reference): displacements (n,3,D,H,W) float32 on the device, in normalised coordinates, n <= 65535 records, the first one
    the centre of the histograms; probs: 2 to 8 increasing probabilities; mask (D,H,W) or None; bins of `bin_width` in the units
    of `scale` (three floats, one per channel; default: voxels).  -> (quantiles (P,3,D,H,W), ci_width (D,H,W), summary dict), as
    diagnostics.DisplacementQuantiles.finalize."""
    from .. import _lib as L
    from ..diagnostics import DisplacementQuantiles
    if displacements.dim() != 5 or displacements.shape[1] != 3:
        raise ValueError(f'displacements must have shape (n, 3, D, H, W), got {tuple(displacements.shape)}')
    dq = DisplacementQuantiles(displacements.shape[2:], displacements.device, bins, bin_width, scale)
    for i in range(0, displacements.shape[0], L.IRS_MAX_CHAINS):  # one launch counts up to IRS_MAX_CHAINS records
        dq.record(displacements[i:i + L.IRS_MAX_CHAINS].float().contiguous())
    return dq.finalize(probs, mask)


@torch.no_grad()
def calc_inverse_consistency(v, transformation_module):
    """Inverse-consistency error of the map a transformation module makes of the velocity v (absent in the reference): v
    (C,3,...) float32 on the device, what `transformation_module` (SVF_3D or SVFFD_3D) takes.  -> {'fixed': |phi^-1 o phi - id|,
    'moving': |phi o phi^-1 - id|, both (C,1,D,H,W) float32 in voxels, 'transformation_inverse', 'displacement_inverse':
    (C,3,D,H,W)}.  For SVFFD_3D the dense velocity is the B-spline up-sampling of v: what the forward exponential integrates."""
    svf = getattr(transformation_module, 'SVF_3D', transformation_module)
    dense = transformation_module.cubic_B_spline_FFD(v) if hasattr(transformation_module, 'cubic_B_spline_FFD') else v
    dense = dense.float().contiguous()
    transformation, displacement = svf(dense)
    t_inv, d_inv = _ops.svf_exp_inverse(dense, getattr(svf, 'no_steps', 12))
    return {'fixed': _ops.inverse_consistency(transformation, displacement, d_inv)[0],
            'moving': _ops.inverse_consistency(t_inv, d_inv, displacement)[0],
            'transformation_inverse': t_inv, 'displacement_inverse': d_inv}


@torch.no_grad()
def calc_DSC_GPU(no_samples, seg_fixed, seg_moving, structures_dict):
    """Dice scores on the device (utils/util.py:123-148)"""
    DSC = torch.zeros(no_samples, len(structures_dict))
    for idx in range(no_samples):
        f, m = seg_fixed[idx], seg_moving[idx]
        for j, label in enumerate(structures_dict.values()):
            num = 2.0 * ((f == label) & (m == label)).sum()
            den = (f == label).sum() + (m == label).sum()
            DSC[idx, j] = num / den  # a label absent from both gives 0 / 0 = NaN, as in the reference (its `except` never fires)
    return DSC.numpy()


@torch.no_grad()
def calc_metrics(seg_fixed, seg_moving, structures_dict, spacing, GPU=True, no_samples=1):
    """average surface distances and Dice scores (utils/util.py:152-206) -> (ASD, DSC), numpy arrays [no_samples, L].
    The ASD runs on the device (ops.label_surface_distance) instead of SimpleITK on the host; `GPU` only chose where the
    reference computed Dice, which is the same number either way."""
    seg_moving = seg_moving[:no_samples].contiguous()
    shared = seg_fixed.shape[0] == 1 or seg_fixed.stride(0) == 0  # one volume, or .expand()-ed chains sharing it
    seg_fixed = seg_fixed[:1].contiguous() if shared else seg_fixed[:no_samples].contiguous()
    ASD = _ops.label_surface_distance(seg_fixed, seg_moving, list(structures_dict.values()), spacing).cpu().numpy()
    DSC = calc_DSC_GPU(no_samples, seg_fixed.expand_as(seg_moving), seg_moving, structures_dict)
    return ASD, DSC


@torch.no_grad()
def calc_surface_metrics(seg_fixed, seg_moving, structures_dict, spacing, percentiles=(95,), no_samples=1):
    """average, Hausdorff and percentile surface distances from one device call (ops.label_hausdorff_distance; the reference
    logs the average only) -> {'ASD': [no_samples, L], 'HD': [no_samples, L], 'HDp': [Q, no_samples, L]}, numpy float64.  The ASD
    is the one calc_metrics returns, bit for bit."""
    seg_moving = seg_moving[:no_samples].contiguous()
    shared = seg_fixed.shape[0] == 1 or seg_fixed.stride(0) == 0  # one volume, or .expand()-ed chains sharing it
    seg_fixed = seg_fixed[:1].contiguous() if shared else seg_fixed[:no_samples].contiguous()
    out = _ops.label_hausdorff_distance(seg_fixed, seg_moving, list(structures_dict.values()), spacing, percentiles)
    return {'ASD': out['asd'].cpu().numpy(), 'HD': out['hd'].cpu().numpy(), 'HDp': out['hd_pct'].cpu().numpy()}


@torch.no_grad()
def calc_native_metrics(displacement, grid, seg_fixed, seg_moving, structures_dict, percentiles=None):
    """Dice scores and surface distances on the image's own voxel grid, in real mm (absent in the reference, which measures on
    the registration grid with a surrogate isotropic spacing): displacement (C,3,*grid.dims) float32 in [-1,1] coordinates;
    grid: a native.NativeGrid; seg_fixed / seg_moving: the UNPADDED native segmentations, (1,1,*grid.shape) int16 on the
    device.  The moving segmentation is carried to the native grid (ops.native_warp, nearest) and compared with the fixed one
    under the header zooms (grid.spacing_xyz()).  -> {'seg': (C,1,*grid.shape) int16, 'DSC': [C, L], 'ASD': [C, L]} and, with
    `percentiles` (a tuple, possibly empty), 'HD': [C, L] and 'HDp': [Q, C, L]; numpy arrays, as calc_metrics /
    calc_surface_metrics return them."""
    seg = _ops.native_warp(displacement, grid, seg=seg_moving)['seg']
    C, spacing = seg.shape[0], grid.spacing_xyz()
    if percentiles is None:
        ASD, DSC = calc_metrics(seg_fixed, seg, structures_dict, spacing, no_samples=C)
        return {'seg': seg, 'DSC': DSC, 'ASD': ASD}
    out = calc_surface_metrics(seg_fixed, seg, structures_dict, spacing, percentiles, no_samples=C)
    fixed = seg_fixed[:1].expand_as(seg) if seg_fixed.shape[0] == 1 else seg_fixed
    return {'seg': seg, 'DSC': calc_DSC_GPU(C, fixed, seg, structures_dict), **out}


@torch.no_grad()
def calc_image_similarity(fixed, moving, mask=None, bins=64, fixed_range=None, moving_range=None):
    """Label-free similarity of the fixed image and a (warped) moving image (absent in the reference): fixed (1 or C,1,D,H,W),
    moving (C,1,D,H,W) float32 on the device, mask (1,1,D,H,W) bool / uint8 or None; the ranges as ops.image_similarity takes
    them.  -> one dict of Python numbers per chain, keyed by ops.SIMILARITY_COLUMNS ('n', 'n_nonfinite', 'n_clipped' as ints;
    'mse', 'ncc', 'h_fixed', 'h_moving', 'h_joint', 'mi', 'nmi' as floats); one host read-back."""
    stats = _ops.image_similarity(fixed, moving, mask, bins, fixed_range, moving_range)['stats'].tolist()
    return [{k: int(x) if j < 3 else x for j, (k, x) in enumerate(zip(_ops.SIMILARITY_COLUMNS, row))} for row in stats]


def local_similarity_rows(stats):
    """the (C,7) stats of ops.local_similarity -> one dict of Python numbers per chain, keyed by ops.LOCAL_COLUMNS ('n', 'n_flat',
    'n_nonfinite' as ints; 'lncc_mean', 'lncc_min', 'ssim_mean', 'ssim_min' as floats); one host read-back"""
    return [{k: int(x) if j < 3 else x for j, (k, x) in enumerate(zip(_ops.LOCAL_COLUMNS, row))} for row in stats.tolist()]


@torch.no_grad()
def calc_local_similarity(fixed, moving, mask=None, radius=2, fixed_range=None, moving_range=None):
    """Statistics of the local similarity maps of the fixed image and a (warped) moving image (absent in the reference): fixed
    (1 or C,1,D,H,W), moving (C,1,D,H,W) float32 on the device, mask (1,1,D,H,W) bool / uint8 or None, radius in 1 .. 4; the
    ranges as ops.local_similarity takes them.  -> one dict per chain (local_similarity_rows); no map is written."""
    return local_similarity_rows(_ops.local_similarity(fixed, moving, mask, radius, fixed_range, moving_range, want=())['stats'])


@torch.no_grad()
def calc_residual_check(residuals, mask, data_loss, half_range, bins=128):
    """Do the residuals look like the likelihood that models them (the numbers behind the reference's log_hist_res figure,
    logger/visualization.py:64-86)?  residuals (C,1,D,H,W) float32 on the device -- the unscaled z of data_loss.map --, mask
    (1,1,D,H,W) bool / uint8 or None, data_loss a GMM or an SSD, bins equal bins over [-half_range, half_range].  -> one dict
    per chain: the entries of residual_check.residual_fit plus 'n_nonfinite' and 'n_clipped'; the three small state tensors are read back."""
    from .. import residual_check as _rc
    half_range = float(torch.tensor(float(half_range), dtype=torch.float32))  # the value the kernel bins with
    out = _rc.residual_histogram(residuals.contiguous(), mask, half_range, bins)
    std, proportions, _, _ = _rc.mixture_terms(data_loss)
    counts = out['counts'].tolist()
    rows = _rc.residual_fit(out['hist'], counts, out['sums'], half_range, std, proportions)
    return [{**row, 'n_nonfinite': int(c[1]), 'n_clipped': int(c[2])} for row, c in zip(rows, counts)]


def calc_native_posterior(displacements, grid, moving_seg=None, structures_dict=None, moving_im=None, fill=None, seg_fixed=None,
                          im_fixed=None, mask=None, std_floor=0.0, voxels=False):
    """The label and / or image posterior on the image's own voxel grid over a list of displacements (absent in the reference):
    the functional form of diagnostics.NativePosterior.  displacements: (C,3,*grid.dims) float32 tensors on the device, one per
    recorded step, in [-1,1] coordinates (`voxels`: in voxels of the registration grid); grid: a native.NativeGrid; moving_seg
    int16 with structures_dict {name: label value} and / or moving_im float32 with its `fill`: the native moving volumes
    (1,1,*grid.shape); seg_fixed / im_fixed / mask: the native fixed segmentation, image (the reference of the z map) and mask.
    -> (what NativePosterior.finalize returns, the recorder itself)"""
    from ..diagnostics import NativePosterior
    displacements = list(displacements)
    if not displacements:
        raise ValueError('calc_native_posterior: no displacement given')
    rec = NativePosterior(grid, displacements[0].device, structures_dict, moving_seg, moving_im, fill, voxels)
    for u in displacements:
        rec.record(u)
    return rec.finalize(seg_fixed, im_fixed, mask, std_floor), rec


def rescale_residuals(res, mask, data_loss):
    """VD-rescaled residual x = sum_k r_k (z / sigma_k)^2 (utils/util.py:330-347).  The reference obtains it as
    sum_k s_k * d(-log p)/d(s_k) with a nested backward; the closed form with the responsibilities r_k is the same number."""
    with torch.no_grad():
        z = torch.where(mask, res, torch.zeros_like(res)).reshape(1, -1, 1)
        s = z * torch.exp(-1.0 * data_loss.log_std)
        t = (data_loss.log_proportions - data_loss.log_std) - 0.5 * s ** 2
        r = torch.softmax(t, dim=-1)
        return torch.sum(r * s * s, dim=-1).view(res.shape)


@torch.no_grad()
def calc_VD_factor(residual, mask):
    """virtual decimation factor from the lag-1 correlations of the rescaled residual (utils/util.py:446-485)"""
    var_res = torch.mean(residual[mask] ** 2)
    n = mask.sum()
    rm = torch.where(mask, residual, torch.zeros_like(residual))
    cov = [torch.sum(rm[:, :, :-1] * rm[:, :, 1:]) / n, torch.sum(rm[:, :, :, :-1] * rm[:, :, :, 1:]) / n,
           torch.sum(rm[:, :, :, :, :-1] * rm[:, :, :, :, 1:]) / n]
    sq = [torch.clamp(-2.0 / math.pi * torch.log(c / var_res), max=1.0) for c in cov]
    return torch.sqrt(sq[0] * sq[1] * sq[2])


@torch.no_grad()
def max_field_update(field_old, field_new):
    """largest voxel-wise update of a vector field in the L2 norm and its index (utils/util.py:281-299)"""
    diff = torch.abs(calc_norm(field_new) - calc_norm(field_old))   # difference of the norms, as the reference defines it
    return torch.max(diff), torch.argmax(diff)


class MetricTracker:
    """running means keyed by name (utils/util.py:488-510 without the pandas dependency)"""

    def __init__(self, *keys, writer=None):
        self.writer = writer
        self._total = {k: 0.0 for k in keys}
        self._count = {k: 0 for k in keys}

    def reset(self):
        for k in self._total:
            self._total[k], self._count[k] = 0.0, 0

    def update(self, key, value, n=1):
        if self.writer is not None:
            self.writer.add_scalar(key, value)
        self._total[key] = self._total.get(key, 0.0) + value * n
        self._count[key] = self._count.get(key, 0) + n

    def avg(self, key):
        return self._total[key] / max(self._count[key], 1)

    def result(self):
        return {k: self.avg(k) for k in self._total}
