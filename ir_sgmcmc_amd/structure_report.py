"""Structure report: what a registration says about one anatomical structure, with error bars.

Every other posterior output is a voxel map, and every summary of one is a number over the mask.  Two per-structure quantities
cannot be derived from the maps afterwards, because the voxels of a structure do not move independently: the spread of the
structure's MEAN displacement over the samples (anywhere between the mean of the per-voxel std map and that divided by
sqrt(voxels)), and the spread of its volume change, sum of det J over its voxels.  Both need one labelled reduction per recorded
sample, on the device, where the displacement and the transformation live:

 - `structure_motion`: per (chain, structure) the voxel and fold counts and the double sums of the displacement, its norm and
   det J, one HIP pass over the sample (include/irsgmcmc.h: irs_structure_motion);
 - `structure_map_stats`: the same labelled reduction over finished per-voxel maps (irs_structure_map_stats);
 - `structure_summary`, `structure_map_rows`: the series of those rows -> the per-structure table, on the host in float64 (a
   few numbers per record and structure: no hot path);
 - the CSV writers of the trainer's two files, and `structure_report_options` / `structure_metric_names` of its option.

The operator wrappers live here and not in ops.py; they use its private helpers.
"""
import math

import numpy as np
import torch

from . import _lib as L
from .modes import split_rhat_series
from .ops import _call, _check_state, _dims5, _labels, _three_positive, _volume_mask, _workspace

MOTION_INT_COLUMNS = ('voxels', 'folded')
MOTION_FLOAT_COLUMNS = ('sum_wx', 'sum_wy', 'sum_wz', 'sum_norm', 'sum_norm2', 'max_norm', 'sum_det', 'min_det', 'max_det')
MAP_INT_COLUMNS = ('finite', 'non_finite')
MAP_FLOAT_COLUMNS = ('sum', 'sum2', 'min', 'max')
# the keys of a structure's motion summary, in the order of the CSV columns and of the metrics; the last two only with the
# displacement covariance recorded beside the report
MOTION_KEYS = ('voxels', 'shift_mean_x', 'shift_mean_y', 'shift_mean_z', 'shift_mean_norm', 'shift_std_major', 'shift_std_minor',
               'shift_std_total', 'disp_mean', 'disp_rms', 'disp_max', 'vol_ratio_mean', 'vol_ratio_std', 'vol_mean_mm3', 'fold_frac',
               'det_min', 'det_max', 'rhat_max')
COHERENCE_KEYS = ('coherence', 'n_eff')
MAP_KEYS = ('mean', 'std', 'min', 'max', 'finite')
SERIES_COLUMNS = ('record', 'step', 'chain', 'structure', 's_x', 's_y', 's_z', 'vol_ratio', 'disp_mean', 'folded')
OPTION_KEYS = ('period', 'maps', 'save')
OPTION_DEFAULTS = {'maps': True, 'save': True}
RHAT_MIN_RECORDS = 4  # per chain: two per half


def _segmentation(seg_fixed, D, H, W):
    if seg_fixed.numel() != D * H * W or tuple(seg_fixed.shape[-3:]) != (D, H, W):
        raise L.IrsError(f'seg_fixed must be a ({D},{H},{W}) volume, got {tuple(seg_fixed.shape)}')
    return seg_fixed.reshape(D, H, W).contiguous()


def structure_motion(displacement, transformation, seg_fixed, labels, scale=(1.0, 1.0, 1.0), mask=None, out=None):
    """One recorded step reduced per structure: displacement (C,3,D,H,W) float32 in voxels and transformation (C,3,D,H,W)
    float32 in [-1,1] coordinates, every chain's sample; seg_fixed (D,H,W) int16 shared by the chains (a leading (1,1) is
    accepted); labels: the K label values; scale: three finite floats > 0, one per channel; mask (D,H,W) bool / uint8 or None.
    -> (ints (C,K,2) int64 MOTION_INT_COLUMNS, floats (C,K,9) float64 MOTION_FLOAT_COLUMNS) on the device.  out: a pair of
    contiguous tensors of those shapes and dtypes to write into -- views into a larger series, say -- instead of new ones.
    No host synchronisation (include/irsgmcmc.h: irs_structure_motion)."""
    Cn, D, H, W = _dims5(displacement, 3)
    _check_state(('transformation', transformation, (Cn, 3, D, H, W), None))
    seg_fixed = _segmentation(seg_fixed, D, H, W)
    lab, K = _labels(labels)
    mask = _volume_mask(mask, D, H, W)
    sc = _three_positive('scale', scale)
    dev = displacement.device
    if out is None:
        out = (torch.empty((Cn, K, L.IRS_STRUCTURE_MOTION_INTS), device=dev, dtype=torch.int64),
               torch.empty((Cn, K, L.IRS_STRUCTURE_MOTION_FLOATS), device=dev, dtype=torch.float64))
    ints, floats = out
    _check_state(('out[0]', ints, (Cn, K, L.IRS_STRUCTURE_MOTION_INTS), torch.int64),
                 ('out[1]', floats, (Cn, K, L.IRS_STRUCTURE_MOTION_FLOATS), torch.float64))
    ws, nbytes = _workspace('irs_structure_workspace', D, H, W, K, Cn, device=dev)
    _call('irs_structure_motion', L.dev_ptr(displacement, torch.float32), L.dev_ptr(transformation, torch.float32), Cn, D, H, W,
          L.dev_ptr(seg_fixed, torch.int16), lab, K, L.dev_ptr(mask, torch.uint8, True), sc, L.dev_ptr(ints), L.dev_ptr(floats),
          L.dev_ptr(ws), nbytes)
    return ints, floats


def structure_map_stats(maps, seg_fixed, labels, mask=None):
    """Per-structure statistics of per-voxel maps: maps (M,D,H,W) float32, any M >= 1; seg_fixed (D,H,W) int16; labels: the K
    label values; mask (D,H,W) bool / uint8 or None.  -> (ints (M,K,2) int64 MAP_INT_COLUMNS, floats (M,K,4) float64
    MAP_FLOAT_COLUMNS over the finite values) on the device.  No host synchronisation (irs_structure_map_stats)."""
    if maps.dim() != 4:
        raise L.IrsError(f'maps must have shape (M,D,H,W), got {tuple(maps.shape)}')
    M, D, H, W = maps.shape
    seg_fixed = _segmentation(seg_fixed, D, H, W)
    lab, K = _labels(labels)
    mask = _volume_mask(mask, D, H, W)
    dev = maps.device
    ints = torch.empty((M, K, L.IRS_STRUCTURE_MAP_INTS), device=dev, dtype=torch.int64)
    floats = torch.empty((M, K, L.IRS_STRUCTURE_MAP_FLOATS), device=dev, dtype=torch.float64)
    ws, nbytes = _workspace('irs_structure_workspace', D, H, W, K, M, device=dev)
    _call('irs_structure_map_stats', L.dev_ptr(maps, torch.float32), M, D, H, W, L.dev_ptr(seg_fixed, torch.int16), lab, K,
          L.dev_ptr(mask, torch.uint8, True), L.dev_ptr(ints), L.dev_ptr(floats), L.dev_ptr(ws), nbytes)
    return ints, floats


# ---------------------------------------------------------------- the host summary (numpy float64)
def _host(t):
    return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)


def record_chains(n, chains):
    """the chain of each of n records ordered by step, then by chain (`chains` per step): r % chains"""
    return np.arange(n) % max(int(chains), 1)


def structure_series(ints, floats):
    """the per-record values behind the summary: ints (n,K,2), floats (n,K,9) -> dict of (n,K) float64 arrays {'voxels',
    'shift' (n,K,3): sum w / voxels, 'disp_mean', 'disp_ms', 'disp_max', 'vol_ratio': sum det / voxels, 'fold_frac', 'det_min',
    'det_max'}; NaN where a structure is empty.  (The columns do not tell how many of a structure's det J were NaN, so the volume
    ratio divides by all its voxels: a NaN det, which only a non-finite transformation gives, counts as 0 there.)"""
    ints = _host(ints).astype(np.int64)
    floats = _host(floats).astype(np.float64)
    vox = ints[..., 0].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        empty = ~(vox > 0)
        vox = np.where(empty, np.nan, vox)
        return {'voxels': ints[..., 0], 'shift': floats[..., 0:3] / vox[..., None], 'disp_mean': floats[..., 3] / vox,
                'disp_ms': floats[..., 4] / vox, 'disp_max': np.where(empty, np.nan, floats[..., 5]),
                'vol_ratio': floats[..., 6] / vox, 'fold_frac': ints[..., 1] / vox, 'det_min': np.where(empty, np.nan, floats[..., 7]),
                'det_max': np.where(empty, np.nan, floats[..., 8])}


def _one_structure(series, j, spacing, chain, cov_trace):
    nan = math.nan
    voxels = int(series['voxels'][0, j])
    n = series['voxels'].shape[0]
    out = dict.fromkeys(MOTION_KEYS, nan)
    out['voxels'] = voxels
    if cov_trace is not None:
        out.update(dict.fromkeys(COHERENCE_KEYS, nan))
    if voxels == 0:
        return out
    s = series['shift'][:, j]
    mean = s.mean(axis=0)
    out['shift_mean_x'], out['shift_mean_y'], out['shift_mean_z'] = (float(v) for v in mean)
    out['shift_mean_norm'] = float(np.sqrt(np.sum(mean * mean)))
    trace = nan
    if n >= 2:
        d = s - mean
        cov = d.T @ d / (n - 1)
        w = np.linalg.eigvalsh(0.5 * (cov + cov.T))
        trace = float(np.trace(cov))
        out['shift_std_major'] = math.sqrt(max(float(w[-1]), 0.0)) if np.isfinite(w).all() else nan
        out['shift_std_minor'] = math.sqrt(max(float(w[0]), 0.0)) if np.isfinite(w).all() else nan
        out['shift_std_total'] = math.sqrt(max(trace, 0.0)) if math.isfinite(trace) else nan
    out['disp_mean'] = float(series['disp_mean'][:, j].mean())
    out['disp_rms'] = float(np.sqrt(series['disp_ms'][:, j].mean()))
    out['disp_max'] = float(np.fmax.reduce(series['disp_max'][:, j]))
    ratio = series['vol_ratio'][:, j]
    out['vol_ratio_mean'] = float(ratio.mean())
    out['vol_ratio_std'] = float(ratio.std(ddof=1)) if n >= 2 else nan
    out['vol_mean_mm3'] = out['vol_ratio_mean'] * voxels * float(np.prod(np.asarray(spacing, dtype=np.float64)))
    out['fold_frac'] = float(series['fold_frac'][:, j].mean())
    out['det_min'] = float(series['det_min'][:, j].min())
    out['det_max'] = float(series['det_max'][:, j].max())
    if chain is not None:
        ids = np.unique(chain)
        counts = [int(np.sum(chain == c)) for c in ids]
        if len(ids) >= 2 and min(counts) >= RHAT_MIN_RECORDS:
            N = min(counts)
            rows = [s[:, 0], s[:, 1], s[:, 2], ratio]
            with np.errstate(invalid='ignore', divide='ignore'):
                rh = [split_rhat_series(np.stack([x[chain == c][:N] for c in ids])) for x in rows]
            out['rhat_max'] = nan if any(math.isnan(r) for r in rh) else float(max(rh))
    if cov_trace is not None:
        denom = float(cov_trace[j])
        with np.errstate(invalid='ignore', divide='ignore'):
            out['coherence'] = float(np.float64(trace) / np.float64(denom)) if n >= 2 else nan
            out['n_eff'] = float(np.float64(1.0) / np.float64(out['coherence']))
    return out


def structure_summary(ints, floats, names, spacing=(1.0, 1.0, 1.0), chains=1, cov_trace=None):
    """The per-structure table from the n records of structure_motion: ints (n,K,2), floats (n,K,9) -- tensors or arrays,
    ordered by step, then by chain; names: the K structure names; spacing: the voxel size behind vol_mean_mm3; chains: records
    per step, or the chain of every record as an array.  -> {'records': n, 'structures': {name: {MOTION_KEYS}}}.  With s_r =
    sum w / voxels of record r: shift_mean_* its mean and the norm of that; shift_std_{major,minor,total} the square roots of the
    largest and smallest eigenvalue and of the trace of its sample covariance (divisor n - 1); disp_mean the mean of sum |w| /
    voxels, disp_rms the root of the mean of sum |w|^2 / voxels, disp_max the largest max |w|; vol_ratio_{mean,std} of sum det /
    voxels and vol_mean_mm3 = vol_ratio_mean voxels prod(spacing); fold_frac the mean of folded / voxels; det_min / det_max over
    the records; rhat_max, with >= 2 chains of >= 4 records, the largest split R-hat (modes.split_rhat_series) of the three
    shift components and the volume ratio.  cov_trace (K,): the mean over the structure's voxels of trace Cov(u(x)) from the
    SAME records adds coherence = trace Cov(s_r) / cov_trace -- 1 for a block, ~ 1 / voxels for independent voxels, <= 1 in exact
    arithmetic and not clamped -- and n_eff = 1 / coherence.  An empty structure gives NaN everywhere but voxels = 0; fewer than
    two records give NaN spreads."""
    series = structure_series(ints, floats)
    n, K = series['voxels'].shape
    names = list(names)
    if n < 1 or len(names) != K:
        raise ValueError(f'structure_summary: {n} records of {K} structures for {len(names)} names')
    chain = np.asarray(chains).reshape(n) if np.ndim(chains) else record_chains(n, chains)
    if cov_trace is not None:
        cov_trace = _host(cov_trace).astype(np.float64).reshape(K)
    return {'records': int(n), 'structures': {name: _one_structure(series, j, spacing, chain, cov_trace) for j, name in enumerate(names)}}


def covariance_trace(ints, floats, n, scale=(1.0, 1.0, 1.0)):
    """the denominator of the coherence from structure_map_stats of the xx, yy, zz co-moment maps of
    diagnostics.DisplacementCovariance after n records: ints (3,K,2), floats (3,K,4) -> (K,) float64, sum_c scale_c^2 sum_x
    comoment_cc(x) / (n - 1) / finite voxels (NaN for an empty structure or n < 2)"""
    ints, floats = _host(ints).astype(np.float64), _host(floats).astype(np.float64)
    s2 = np.asarray(scale, dtype=np.float64).reshape(3, 1) ** 2
    with np.errstate(invalid='ignore', divide='ignore'):
        return (s2 * floats[:, :, 0] / ints[:, :, 0]).sum(axis=0) / (n - 1) if n >= 2 else np.full(ints.shape[1], np.nan)


def structure_map_rows(ints, floats, map_names, names):
    """ints (M,K,2), floats (M,K,4) of structure_map_stats -> {structure: {'{map}_mean', '{map}_std' (spatial, divisor = finite
    count, the variance clamped at 0), '{map}_min', '{map}_max', '{map}_finite'}}; a structure without a finite value of a map
    gives NaN and finite = 0"""
    ints, floats = _host(ints).astype(np.int64), _host(floats).astype(np.float64)
    out = {}
    for j, name in enumerate(names):
        row = {}
        for m, key in enumerate(map_names):
            k = int(ints[m, j, 0])
            if k > 0:
                mean = floats[m, j, 0] / k
                row.update({f'{key}_mean': float(mean), f'{key}_std': math.sqrt(max(float(floats[m, j, 1] / k - mean * mean), 0.0)),
                            f'{key}_min': float(floats[m, j, 2]), f'{key}_max': float(floats[m, j, 3])})
            else:
                row.update({f'{key}_{stat}': math.nan for stat in MAP_KEYS[:4]})
            row[f'{key}_finite'] = k
        out[name] = row
    return out


def add_map_rows(summary, rows, map_names):
    """the rows of structure_map_rows appended to every structure of a structure_summary, and `map_names` as summary['maps'];
    a map whose columns would replace a motion key ('rhat' would: rhat_max) is refused"""
    for name, row in rows.items():
        taken = set(row) & set(summary['structures'][name])
        if taken:
            raise ValueError(f'structure report: map columns {sorted(taken)} are keys of the motion summary already')
        summary['structures'][name].update(row)
    summary['maps'] = list(map_names)
    return summary


# ---------------------------------------------------------------- the trainer's option, metric names and files
def structure_report_options(cfg_trainer, data_loader=None, structures=None):
    """`trainer.structure_report` -> None when off, else {'period': P, 'maps': bool, 'save': bool}.
    Absent / false / null: off.  true: P = log_period_MCMC, the per-structure rows of every posterior map, files written.
    {"period": P, "maps": bool, "save": bool}: any key may be left out.  Refuses unknown keys, a non-integer P or P < 1, values
    of "maps" / "save" that are no booleans, and a config that records no step (no_samples_MCMC // P < 1); with the option on,
    also a `data_loader` that found no segmentations and an empty `structures` (None: not checked)."""
    from .diagnostics import MAX_RECORDS, _record_options

    def own_keys(opt):
        out = dict(OPTION_DEFAULTS)
        for key in out:
            if key in opt:
                if not isinstance(opt[key], bool):
                    raise ValueError(f'trainer.structure_report.{key} must be true or false, got {opt[key]!r}')
                out[key] = opt[key]
        return out

    out = _record_options(cfg_trainer, 'structure_report', OPTION_KEYS, '{"period": P, "maps": true, "save": true}', MAX_RECORDS,
                          'the series holds at most {}', own_keys)
    if out is not None and data_loader is not None and not getattr(data_loader, 'has_segs', True):
        raise ValueError(f'trainer.structure_report needs the fixed segmentation, and the data loader '
                         f'({type(data_loader).__name__}) found no "segs" directory')
    if out is not None and structures is not None and not structures:
        raise ValueError('trainer.structure_report needs structures (the config lists none)')
    return out


def with_coherence(cfg_trainer):
    """whether the report carries coherence / n_eff: trainer.displacement_covariance is on with the report's period, so that
    both have seen the same records"""
    from .diagnostics import displacement_covariance_options
    opt, cov = structure_report_options(cfg_trainer), displacement_covariance_options(cfg_trainer)
    return opt is not None and cov is not None and cov['period'] == opt['period']


def structure_metric_keys(cfg_trainer):
    return MOTION_KEYS + (COHERENCE_KEYS if with_coherence(cfg_trainer) else ())


def structure_metric_names(cfg_trainer, structures):
    """MCMC/structure/{key}/{structure} for the motion keys, structure by structure"""
    return [f'MCMC/structure/{key}/{s}' for s in structures for key in structure_metric_keys(cfg_trainer)]


def _cell(v):
    return str(int(v)) if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else repr(float(v))


def structures_csv(summary):
    """(header, rows) of samples/MCMC_structures.csv: one row per structure, the motion columns then the map columns, integers
    as integers and floats by repr (they read back exactly)"""
    rows, header = [], None
    for name, row in summary['structures'].items():
        if header is None:
            header = ['structure'] + list(row)
        rows.append([name] + [_cell(row[k]) for k in header[1:]])
    return header or ['structure'], rows


def series_csv(ints, floats, names, steps, chains):
    """(header, rows) of samples/MCMC_structure_series.csv: per record and structure SERIES_COLUMNS -- the record's number, the
    transition it was taken at, its chain, the structure, s = sum w / voxels, the volume ratio, the mean |w| and the folded
    voxels"""
    series = structure_series(ints, floats)
    folded = _host(ints).astype(np.int64)[..., 1]
    n, K = folded.shape
    rows = []
    for r in range(n):
        for j, name in enumerate(names):
            rows.append([str(r), str(int(steps[r // chains])), str(r % chains), name] +
                        [repr(float(v)) for v in (*series['shift'][r, j], series['vol_ratio'][r, j], series['disp_mean'][r, j])] +
                        [str(int(folded[r, j]))])
    return list(SERIES_COLUMNS), rows


def write_csv(file_path, header, rows):
    with open(file_path, 'w', newline='\n') as f:
        f.write(','.join(header) + '\n')
        for row in rows:
            f.write(','.join(row) + '\n')


def read_csv(file_path):
    """-> (header, rows of cells: int where the cell is an integer, else float where it is one, else the string)"""
    def cell(c):
        try:
            return int(c)
        except ValueError:
            try:
                return float(c)
            except ValueError:
                return c
    with open(file_path) as f:
        lines = [line.rstrip('\n').split(',') for line in f if line.strip()]
    return lines[0], [[cell(c) for c in line] for line in lines[1:]]
