"""Observability for the MCMC path: console/file logging, a scalar writer, and the reference's file writers.

The TensorBoard / seaborn figures of the reference's logger are out of scope; its output FILES
are not: `save_im_to_disk` (.nii.gz), `save_field_to_disk` / `save_grid_to_disk` (.vtk) and the helpers built on them
(logger/logger.py:35-240) are reproduced on top of utils/imageio.py (numpy; no nibabel / tvtk).
"""
import logging
from os import path

import numpy as np

from ..utils.imageio import write_nifti, write_vtk_field, write_vtk_grid, write_vtk_points


def setup_logging(save_dir=None, level=logging.INFO):
    handlers = [logging.StreamHandler()]
    if save_dir is not None:
        handlers.append(logging.FileHandler(str(save_dir) + '/info.log'))
    logging.basicConfig(level=level, format='%(message)s', handlers=handlers, force=True)


class ScalarWriter:
    """stand-in for TensorboardWriter (logger/visualization.py:12-55): remembers the last value of every scalar"""

    def __init__(self):
        self.step = 0
        self.scalars = {}

    def set_step(self, step):
        self.step = step

    def add_scalar(self, key, value):
        self.scalars[key] = (self.step, value)

    def write_hparams(self, *_):
        pass


# ------------------------------------------------------------------ file writers (logger/logger.py:35-240)
def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def save_field_to_disk(field, file_path, spacing=(1, 1, 1)):
    """vector field (3, nx, ny, nz) -> legacy .vtk, x fastest (logger/logger.py:35-60)"""
    write_vtk_field(_np(field), file_path, _np(spacing))


def save_grid_to_disk(grid, file_path):
    """sampling grid (3, nx, ny, nz) -> .vtk structured grid (logger/logger.py:63-80)"""
    write_vtk_grid(_np(grid), file_path)


def save_im_to_disk(im, file_path, spacing=(1, 1, 1)):
    """3-D image -> .nii.gz with identity affine, mm units, zooms = spacing (logger/logger.py:83-100)"""
    write_nifti(_np(im), file_path, _np(spacing))


def _folder(save_dirs, key, model=None):
    import os
    folder = path.join(str(save_dirs['samples']), model) if model is not None else str(save_dirs[key])
    os.makedirs(folder, exist_ok=True)
    return folder


def save_field(save_dirs, spacing, field, field_name, model=None):
    save_field_to_disk(field, path.join(_folder(save_dirs, 'fields', model), f'{field_name}.vtk'), spacing)


def save_im(save_dirs, spacing, im, name, model=None):
    save_im_to_disk(im, path.join(_folder(save_dirs, 'images', model), f'{name}.nii.gz'), spacing)


def save_fixed_im(save_dirs, spacing, im_fixed):
    save_im(save_dirs, spacing, im_fixed[0, 0], 'im_fixed')


def save_fixed_mask(save_dirs, spacing, mask_fixed):
    save_im(save_dirs, spacing, mask_fixed[0, 0].float(), 'mask_fixed')


def save_moving_im(save_dirs, spacing, im_moving_batch):
    save_im(save_dirs, spacing, im_moving_batch[0, 0], 'im_moving')


def save_moving_mask(save_dirs, spacing, mask_moving):
    save_im(save_dirs, spacing, mask_moving[0, 0].float(), 'mask_moving')


def save_displacement_mean_and_std_dev(logger, save_dirs, spacing, displacement_mean, displacement_std_dev, mask, model):
    """posterior mean / std of the displacement in mm, plain and masked (logger/logger.py:110-131)"""
    folder = _folder(save_dirs, 'samples')
    for name, field in (('mean', displacement_mean), ('std_dev', displacement_std_dev)):
        field = field * spacing[0]
        logger.info(f'{model} displacement {name.replace("_", ". ")} min.: {float(field.min()):.2f}, max.: {float(field.max()):.2f}')
        save_field_to_disk(field, path.join(folder, f'{model}_sample_{name}.vtk'), spacing)
        save_field_to_disk(field * mask[0], path.join(folder, f'{model}_sample_{name}_masked.vtk'), spacing)


def save_sample(save_dirs, spacing, sample_no, im_moving_warped_batch, displacement_batch, log_det_J_batch, model, chain_no=None):
    """warped image, displacement (mm) and log det J of one sample (logger/logger.py:215-240)"""
    prefix = f'chain_{chain_no}_sample_{sample_no:07}' if model == 'MCMC' else f'sample_{sample_no:07}'
    save_im(save_dirs, spacing, im_moving_warped_batch[0, 0], f'{prefix}_im_moving_warped', model)
    save_field(save_dirs, spacing, displacement_batch[0] * spacing[0], f'{prefix}_displacement', model)
    save_im(save_dirs, spacing, log_det_J_batch[0], f'{prefix}_log_det_J', model)


def save_precond_sigma(logger, save_dirs, spacing, sigma_rms, mask, model='MCMC'):
    """the frozen sigma field of the adaptive preconditioner (absent in the reference), per voxel the RMS of its three channels,
    plain and masked as the std map is: samples/{model}_precond_sigma.nii.gz and samples/{model}_precond_sigma_masked.nii.gz"""
    folder = _folder(save_dirs, 'samples')
    mask = mask.reshape(sigma_rms.shape).to(sigma_rms.device) != 0
    logger.info(f'{model} preconditioner sigma (RMS over the channels) min.: {float(sigma_rms.min()):.4f}, max.: '
                f'{float(sigma_rms.max()):.4f}')
    save_im_to_disk(sigma_rms, path.join(folder, f'{model}_precond_sigma.nii.gz'), spacing)
    save_im_to_disk(sigma_rms.where(mask, sigma_rms.new_zeros(())), path.join(folder, f'{model}_precond_sigma_masked.nii.gz'), spacing)


def save_rhat(logger, save_dirs, spacing, rhat, mask, model='MCMC'):
    """split-R-hat map of the displacement (absent in the reference), plain and masked as the std map is:
    samples/{model}_rhat.nii.gz and samples/{model}_rhat_masked.nii.gz (0 outside the mask)"""
    folder = _folder(save_dirs, 'samples')
    mask = mask.reshape(rhat.shape).to(rhat.device) != 0
    logger.info(f'{model} split R-hat min.: {float(rhat.min()):.4f}, max.: {float(rhat.max()):.4f}')
    save_im_to_disk(rhat, path.join(folder, f'{model}_rhat.nii.gz'), spacing)
    save_im_to_disk(rhat.where(mask, rhat.new_zeros(())), path.join(folder, f'{model}_rhat_masked.nii.gz'), spacing)


def save_ess(logger, save_dirs, spacing, ess, mcse, mask, model='MCMC'):
    """split ESS and MCSE maps of the displacement (absent in the reference), plain and masked as the std map is:
    samples/{model}_ess[_masked].nii.gz and samples/{model}_mcse[_masked].nii.gz (0 outside the mask)"""
    folder = _folder(save_dirs, 'samples')
    mask = mask.reshape(ess.shape).to(ess.device) != 0
    logger.info(f'{model} split ESS min.: {float(ess.min()):.1f}, max.: {float(ess.max()):.1f}; '
                f'MCSE max.: {float(mcse.max()):.4g}')
    for name, im in (('ess', ess), ('mcse', mcse)):
        save_im_to_disk(im, path.join(folder, f'{model}_{name}.nii.gz'), spacing)
        save_im_to_disk(im.where(mask, im.new_zeros(())), path.join(folder, f'{model}_{name}_masked.nii.gz'), spacing)


def save_label_posterior(logger, save_dirs, spacing, entropy, map_label, mask, prob=None, names=(), model='MCMC'):
    """posterior label maps of the propagated segmentation (absent in the reference): samples/{model}_seg_entropy.nii.gz,
    {model}_seg_entropy_masked.nii.gz (0 outside the FIXED mask), {model}_seg_MAP.nii.gz (int16) and, with `prob` (K,D,H,W),
    {model}_seg_prob_{name}.nii.gz (float32) per structure"""
    folder = _folder(save_dirs, 'samples')
    mask = mask.reshape(entropy.shape).to(entropy.device) != 0
    logger.info(f'{model} segmentation entropy max.: {float(entropy.max()):.4f} nats')
    save_im_to_disk(entropy, path.join(folder, f'{model}_seg_entropy.nii.gz'), spacing)
    save_im_to_disk(entropy.where(mask, entropy.new_zeros(())), path.join(folder, f'{model}_seg_entropy_masked.nii.gz'), spacing)
    save_im_to_disk(map_label, path.join(folder, f'{model}_seg_MAP.nii.gz'), spacing)
    if prob is not None:
        for name, p in zip(names, prob):
            save_im_to_disk(p, path.join(folder, f'{model}_seg_prob_{name}.nii.gz'), spacing)


def save_jacobian_posterior(logger, save_dirs, spacing, fold_prob, logJ_mean, logJ_std, mask, model='MCMC'):
    """Jacobian posterior maps (absent in the reference): samples/{model}_fold_prob.nii.gz, {model}_logJ_mean[_masked].nii.gz
    and {model}_logJ_std[_masked].nii.gz (float32; the masked ones 0 outside the FIXED mask; NaN where every record folds)"""
    folder = _folder(save_dirs, 'samples')
    mask = mask.reshape(fold_prob.shape).to(fold_prob.device) != 0
    logger.info(f'{model} fold probability max.: {float(fold_prob.max()):.4f}')
    save_im_to_disk(fold_prob, path.join(folder, f'{model}_fold_prob.nii.gz'), spacing)
    for name, im in (('logJ_mean', logJ_mean), ('logJ_std', logJ_std)):
        save_im_to_disk(im, path.join(folder, f'{model}_{name}.nii.gz'), spacing)
        save_im_to_disk(im.where(mask, im.new_zeros(())), path.join(folder, f'{model}_{name}_masked.nii.gz'), spacing)


def save_image_posterior(logger, save_dirs, spacing, maps, mask, model='MCMC'):
    """the image posterior (absent in the reference): per volume `name` of `maps` (diagnostics.ImagePosterior.finalize)
    samples/{model}_im_{name}_{mean,std,range}[_masked].nii.gz and, where it holds a z map, {model}_im_{name}_z[_masked].nii.gz
    (float32; NaN -- a non-finite sample there -- written as 0, the masked ones 0 outside the FIXED mask too)"""
    folder = _folder(save_dirs, 'samples')
    for name, volume in maps.items():
        for key in ('mean', 'std', 'range', 'z'):
            if key not in volume:
                continue
            im, undefined = _nan_to_zero(volume[key])
            m = mask.reshape(im.shape).to(im.device) != 0
            logger.info(f'{model}_im_{name}_{key}: {undefined} voxels without a finite value written as 0')
            save_im_to_disk(im, path.join(folder, f'{model}_im_{name}_{key}.nii.gz'), spacing)
            save_im_to_disk(im.where(m, im.new_zeros(())), path.join(folder, f'{model}_im_{name}_{key}_masked.nii.gz'), spacing)


def save_displacement_covariance(logger, save_dirs, spacing, std, direction, anisotropy, mask, model='MCMC'):
    """principal spread of the displacement posterior (absent in the reference): samples/{model}_disp_std_major[_masked].nii.gz,
    {model}_disp_std_minor[_masked].nii.gz and {model}_disp_anisotropy[_masked].nii.gz (float32, the std in the units of the
    finalize's scale; the masked ones 0 outside the mask), and samples/{model}_disp_direction.vtk: the major direction scaled
    by the major std, as a field"""
    folder = _folder(save_dirs, 'samples')
    mask = mask.reshape(anisotropy.shape).to(anisotropy.device) != 0
    logger.info(f'{model} displacement major std max.: {float(std[0].max()):.4f}, anisotropy max.: {float(anisotropy.max()):.4f}')
    for name, im in (('disp_std_major', std[0]), ('disp_std_minor', std[2]), ('disp_anisotropy', anisotropy)):
        save_im_to_disk(im, path.join(folder, f'{model}_{name}.nii.gz'), spacing)
        save_im_to_disk(im.where(mask, im.new_zeros(())), path.join(folder, f'{model}_{name}_masked.nii.gz'), spacing)
    save_field_to_disk(direction * std[0], path.join(folder, f'{model}_disp_direction.vtk'), spacing)


def save_displacement_modes(logger, save_dirs, spacing, out, mask, model='MCMC'):
    """principal modes of the displacement posterior (absent in the reference), `out` as diagnostics.DisplacementModes.finalize
    returns it: samples/{model}_mode_{k}.vtk, k = 1 .. K, the 1-sigma mode field written the way the mean displacement is;
    {model}_modes_explained[_masked].nii.gz (float32, the masked one 0 outside the mask); {model}_modes.csv (m, eigenvalue,
    share, cumulative share, split R-hat of the scores) and {model}_mode_scores.csv (record, step, chain, one score per mode)"""
    folder = _folder(save_dirs, 'samples')
    explained = out['explained_map']
    mask = mask.reshape(explained.shape).to(explained.device) != 0
    logger.info(f'{model} explained-variance map of {out["modes"].shape[0]} modes min.: {float(explained.min()):.4f}, max.: '
                f'{float(explained.max()):.4f}')
    for k, field in enumerate(out['modes'], start=1):
        save_field_to_disk(field * spacing[0], path.join(folder, f'{model}_mode_{k}.vtk'), spacing)
    save_im_to_disk(explained, path.join(folder, f'{model}_modes_explained.nii.gz'), spacing)
    save_im_to_disk(explained.where(mask, explained.new_zeros(())), path.join(folder, f'{model}_modes_explained_masked.nii.gz'), spacing)
    K = out['scores'].shape[1]
    cumulative = np.cumsum(out['explained'])
    with open(path.join(folder, f'{model}_modes.csv'), 'w') as f:
        f.write('m,eigenvalue,share,cumulative_share,rhat\n')
        for m in range(K):
            f.write(f'{m + 1},{out["eigenvalues"][m]:.17g},{out["explained"][m]:.17g},{cumulative[m]:.17g},{out["rhat"][m]:.6g}\n')
    with open(path.join(folder, f'{model}_mode_scores.csv'), 'w') as f:
        f.write('record,step,chain,' + ','.join(f'score_{m + 1}' for m in range(K)) + '\n')
        for i, (step, chain) in enumerate(zip(out['steps'], out['chains'])):
            f.write(f'{i},{step},{chain},' + ','.join(f'{v:.17g}' for v in out['scores'][i]) + '\n')


def save_displacement_quantiles(logger, save_dirs, spacing, probs, quantiles, ci_width, mask, model='MCMC'):
    """credible intervals of the displacement posterior (absent in the reference): samples/{model}_disp_q{PP}.vtk, one field
    per probability (PP the probability in percent, `g` formatting, the dot replaced by `p`: q5, q50, q95, q2p5; NaN where out
    of range), and samples/{model}_disp_ci_width[_masked].nii.gz (float32, in the units of the quantiles; the masked one 0
    outside the mask)"""
    folder = _folder(save_dirs, 'samples')
    mask = mask.reshape(ci_width.shape).to(ci_width.device) != 0
    finite = ci_width[~ci_width.isnan()]
    logger.info(f'{model} displacement credible band width max.: {float(finite.max()) if finite.numel() else float("nan"):.4f}')
    for p, q in zip(probs, quantiles):
        save_field_to_disk(q, path.join(folder, f'{model}_disp_q{quantile_tag(p)}.vtk'), spacing)
    save_im_to_disk(ci_width, path.join(folder, f'{model}_disp_ci_width.nii.gz'), spacing)
    save_im_to_disk(ci_width.where(mask, ci_width.new_zeros(())), path.join(folder, f'{model}_disp_ci_width_masked.nii.gz'), spacing)


def quantile_tag(p):
    """0.05 -> '5', 0.5 -> '50', 0.025 -> '2p5'"""
    return f'{100.0 * float(p):g}'.replace('.', 'p')


def save_inverse_consistency(logger, save_dirs, spacing, mean, peak, masks, model='MCMC'):
    """inverse-consistency error maps in voxels (absent in the reference): samples/{model}_ICE_{fixed,moving}_{mean,max}
    [_masked].nii.gz (float32).  `mean` / `peak` / `masks`: dicts with the keys 'fixed' (|phi^-1 o phi - id| on the fixed grid,
    masked by the FIXED mask) and 'moving' (|phi o phi^-1 - id| on the moving grid, masked by the MOVING mask); the masked maps
    are 0 outside their mask"""
    folder = _folder(save_dirs, 'samples')
    for space in ('fixed', 'moving'):
        mask = masks[space].reshape(mean[space].shape).to(mean[space].device) != 0
        for name, im in (('mean', mean[space]), ('max', peak[space])):
            save_im_to_disk(im, path.join(folder, f'{model}_ICE_{space}_{name}.nii.gz'), spacing)
            save_im_to_disk(im.where(mask, im.new_zeros(())), path.join(folder, f'{model}_ICE_{space}_{name}_masked.nii.gz'), spacing)


def save_native_sample(save_dirs, zooms, sample_no, chain_no, im=None, seg=None, displacement_mm=None, model='MCMC'):
    """one sample on the image's own voxel grid (absent in the reference): samples/{model}/chain_{c}_sample_{N}
    _im_moving_warped_native.nii.gz (float32), _seg_moving_warped_native.nii.gz (int16) and _displacement_native.vtk (mm), each
    when given; `zooms`: the header zooms in the axis order of the arrays, written as the files' spacing"""
    prefix = f'chain_{chain_no}_sample_{sample_no:07}'
    if im is not None:
        save_im(save_dirs, zooms, im, f'{prefix}_im_moving_warped_native', model)
    if seg is not None:
        save_im(save_dirs, zooms, seg, f'{prefix}_seg_moving_warped_native', model)
    if displacement_mm is not None:
        save_field(save_dirs, zooms, displacement_mm, f'{prefix}_displacement_native', model)


def save_native_mean(logger, save_dirs, zooms, displacement_mm, im_warped, model='MCMC'):
    """the posterior-mean displacement carried to the image's own voxel grid, in mm, and the native moving image warped by it
    (absent in the reference): samples/{model}_sample_mean_native.vtk and samples/{model}_im_moving_warped_mean_native.nii.gz"""
    folder = _folder(save_dirs, 'samples')
    logger.info(f'{model} native displacement mean min.: {float(displacement_mm.min()):.2f}, max.: {float(displacement_mm.max()):.2f} mm')
    save_field_to_disk(displacement_mm, path.join(folder, f'{model}_sample_mean_native.vtk'), zooms)
    save_im_to_disk(im_warped, path.join(folder, f'{model}_im_moving_warped_mean_native.nii.gz'), zooms)


def save_native_posterior(logger, save_dirs, zooms, maps, prob=None, names=(), model='MCMC'):
    """the posteriors on the image's own voxel grid (absent in the reference), `maps` as diagnostics.NativePosterior.finalize
    returns them: samples/{model}_seg_{entropy,MAP}_native.nii.gz (float32 / int16), with `prob` (K, *native shape)
    {model}_seg_prob_{name}_native.nii.gz per structure, and samples/{model}_im_moving_{mean,std,range,z}_native.nii.gz (float32;
    NaN -- a non-finite sample there -- written as 0).  `zooms`: the header zooms in the axis order of the arrays, written as
    the files' spacing"""
    folder = _folder(save_dirs, 'samples')
    if 'labels' in maps:
        logger.info(f'{model} native segmentation entropy max.: {float(maps["labels"]["entropy"].max()):.4f} nats')
        save_im_to_disk(maps['labels']['entropy'], path.join(folder, f'{model}_seg_entropy_native.nii.gz'), zooms)
        save_im_to_disk(maps['labels']['map'], path.join(folder, f'{model}_seg_MAP_native.nii.gz'), zooms)
        if prob is not None:
            for name, p in zip(names, prob):
                save_im_to_disk(p, path.join(folder, f'{model}_seg_prob_{name}_native.nii.gz'), zooms)
    if 'image' in maps:
        for key in ('mean', 'std', 'range', 'z'):
            if key in maps['image']:
                im, undefined = _nan_to_zero(maps['image'][key])
                logger.info(f'{model}_im_moving_{key}_native: {undefined} voxels without a finite value written as 0')
                save_im_to_disk(im, path.join(folder, f'{model}_im_moving_{key}_native.nii.gz'), zooms)


def save_landmarks(logger, save_dirs, mean_points, table, columns, unit, model='MCMC', tag=''):
    """the landmark posterior (absent in the reference): samples/{model}_landmarks{tag}.csv, one row per landmark under a header
    line -- the posterior-mean mapped point (x, y, z) and the columns of ops.LANDMARK_COLUMNS, in `unit` -- and
    samples/{model}_landmarks{tag}_mean.vtk, the mean points as legacy ASCII POLYDATA with the point scalars tre_of_mean,
    std_major and pit"""
    folder = _folder(save_dirs, 'samples')
    mean_points, table, columns = _np(mean_points), _np(table), list(columns)
    with open(path.join(folder, f'{model}_landmarks{tag}.csv'), 'w', newline='\n') as f:
        f.write(','.join(['landmark', 'mean_x', 'mean_y', 'mean_z'] + columns) + '\n')
        for k, (pt, row) in enumerate(zip(mean_points, table)):
            f.write(','.join([str(k)] + [repr(float(v)) for v in pt] + [repr(float(v)) for v in row]) + '\n')
    write_vtk_points(mean_points, path.join(folder, f'{model}_landmarks{tag}_mean.vtk'),
                     [(name, table[:, columns.index(name)]) for name in ('tre_of_mean', 'std_major', 'pit')],
                     title=f'posterior-mean landmarks ({unit})')
    logger.info(f'{model} landmarks{tag}: {len(table)} rows in {unit} -> {model}_landmarks{tag}.csv, {model}_landmarks{tag}_mean.vtk')


def save_structure_report(logger, save_dirs, table, series, model='MCMC'):
    """the structure report (absent in the reference): samples/{model}_structures.csv, one row per structure -- the motion
    columns, then the map columns -- and samples/{model}_structure_series.csv, one row per record and structure; `table` and
    `series` are the (header, rows) of structure_report.structures_csv / series_csv (floats by repr: they read back exactly)"""
    from ..structure_report import write_csv
    folder = _folder(save_dirs, 'samples')
    write_csv(path.join(folder, f'{model}_structures.csv'), *table)
    write_csv(path.join(folder, f'{model}_structure_series.csv'), *series)
    logger.info(f'{model} structure report: {len(table[1])} structures, {len(series[1])} series rows -> {model}_structures.csv, '
                f'{model}_structure_series.csv')


def save_truth_calibration(logger, save_dirs, spacing, maps, mask, calibration, series, model='MCMC'):
    """the known-transformation validation (absent in the reference): samples/{model}_truth_{error,mahalanobis}[_masked].nii.gz
    (float32; NaN -- a non-finite state or truth there -- written as 0, the masked ones 0 outside the mask too),
    samples/{model}_truth_calibration.csv and samples/{model}_truth_series.csv; `calibration` and `series` are the (header, rows)
    of truth.calibration_csv / series_csv (floats by repr: they read back exactly)"""
    from ..structure_report import write_csv
    folder = _folder(save_dirs, 'samples')
    for name in ('error', 'mahalanobis'):
        im, undefined = _nan_to_zero(maps[name])
        m = mask.reshape(im.shape).to(im.device) != 0
        logger.info(f'{model}_truth_{name}: {undefined} voxels with a non-finite state written as 0')
        save_im_to_disk(im, path.join(folder, f'{model}_truth_{name}.nii.gz'), spacing)
        save_im_to_disk(im.where(m, im.new_zeros(())), path.join(folder, f'{model}_truth_{name}_masked.nii.gz'), spacing)
    write_csv(path.join(folder, f'{model}_truth_calibration.csv'), *calibration)
    write_csv(path.join(folder, f'{model}_truth_series.csv'), *series)
    logger.info(f'{model} truth calibration: {len(calibration[1])} table rows, {len(series[1])} series rows -> '
                f'{model}_truth_calibration.csv, {model}_truth_series.csv')


def _nan_to_zero(im):
    """-> (the map with 0 where it is NaN, how many voxels that was)"""
    nan = im.isnan()
    return im.where(~nan, im.new_zeros(())), int(nan.sum())


def save_local_similarity_posterior(logger, save_dirs, spacing, mean, low, mask, model='MCMC'):
    """the posterior of the LNCC maps (absent in the reference): samples/{model}_lncc_{mean,min}[_masked].nii.gz (float32; NaN --
    no sample was defined there -- written as 0, the masked ones 0 outside the mask too)"""
    folder = _folder(save_dirs, 'samples')
    mask = mask.reshape(mean.shape).to(mean.device) != 0
    for name, im in (('lncc_mean', mean), ('lncc_min', low)):
        im, undefined = _nan_to_zero(im)
        logger.info(f'{model}_{name}: {undefined} voxels without a defined sample written as 0')
        save_im_to_disk(im, path.join(folder, f'{model}_{name}.nii.gz'), spacing)
        save_im_to_disk(im.where(mask, im.new_zeros(())), path.join(folder, f'{model}_{name}_masked.nii.gz'), spacing)


def save_local_similarity_of_mean(logger, save_dirs, spacing, lncc, ssim, model='MCMC'):
    """the local similarity maps of the moving image under the posterior-mean displacement (absent in the reference):
    samples/{model}_lncc_of_mean.nii.gz and samples/{model}_ssim_of_mean.nii.gz (float32; NaN written as 0)"""
    folder = _folder(save_dirs, 'samples')
    for name, im in (('lncc', lncc), ('ssim', ssim)):
        im, undefined = _nan_to_zero(im)
        logger.info(f'{model}_{name}_of_mean: {undefined} undefined voxels written as 0')
        save_im_to_disk(im, path.join(folder, f'{model}_{name}_of_mean.nii.gz'), spacing)


def residual_histogram_rows(edges, hist, model_probability):
    """the table of samples/{model}_residual_hist.csv: header, then one row per bin -- bin_lo, bin_hi, the count of every
    chain, their sum, and the mixture's mass in the bin"""
    hist = _np(hist)
    header = ['bin_lo', 'bin_hi'] + [f'count_chain_{i}' for i in range(hist.shape[0])] + ['count', 'model_probability']
    rows = [[repr(float(edges[b])), repr(float(edges[b + 1]))] + [str(int(c)) for c in hist[:, b]] +
            [str(int(hist[:, b].sum())), repr(float(model_probability[b]))] for b in range(hist.shape[1])]
    return header, rows


def save_residual_histogram(logger, save_dirs, edges, hist, model_probability, model='MCMC'):
    """the recorded residual histogram against the mixture (the numbers behind the reference's log_hist_res figure):
    samples/{model}_residual_hist.csv, residual_histogram_rows"""
    folder = _folder(save_dirs, 'samples')
    header, rows = residual_histogram_rows(edges, hist, model_probability)
    with open(path.join(folder, f'{model}_residual_hist.csv'), 'w', newline='\n') as f:
        f.write(','.join(header) + '\n')
        for row in rows:
            f.write(','.join(row) + '\n')
    logger.info(f'{model} residual histogram: {len(rows)} bins -> {model}_residual_hist.csv')


def save_residual_nll(logger, save_dirs, spacing, mean, mask, model='MCMC'):
    """the posterior mean of the per-voxel negative log-likelihood: samples/{model}_nll_mean[_masked].nii.gz (float32; NaN -- no
    finite residual there -- written as 0, the masked one 0 outside the mask too)"""
    folder = _folder(save_dirs, 'samples')
    mask = mask.reshape(mean.shape).to(mean.device) != 0
    im, undefined = _nan_to_zero(mean)
    logger.info(f'{model}_nll_mean: {undefined} voxels without a finite residual written as 0')
    save_im_to_disk(im, path.join(folder, f'{model}_nll_mean.nii.gz'), spacing)
    save_im_to_disk(im.where(mask, im.new_zeros(())), path.join(folder, f'{model}_nll_mean_masked.nii.gz'), spacing)


def save_posterior_comparison(logger, save_dirs, spacing, maps, mask, model='MCMC'):
    """the VI posterior against the MCMC samples (absent in the reference): samples/{model}_vs_VI_{shift,log_std_ratio,bures,
    jeffreys}[_masked].nii.gz (float32; NaN -- a non-finite state there -- written as 0, the masked ones 0 outside the mask too).
    `maps`: the dict of diagnostics.PosteriorComparison.finalize"""
    folder = _folder(save_dirs, 'samples')
    for name in ('shift', 'log_std_ratio', 'bures', 'jeffreys'):
        im, undefined = _nan_to_zero(maps[name])
        m = mask.reshape(im.shape).to(im.device) != 0
        logger.info(f'{model}_vs_VI_{name}: {undefined} voxels with a non-finite state written as 0')
        save_im_to_disk(im, path.join(folder, f'{model}_vs_VI_{name}.nii.gz'), spacing)
        save_im_to_disk(im.where(m, im.new_zeros(())), path.join(folder, f'{model}_vs_VI_{name}_masked.nii.gz'), spacing)


def save_surface_posterior(logger, save_dirs, spacing, bias, std, model='MCMC'):
    """the surface posterior (absent in the reference): samples/{model}_surface_bias.nii.gz and samples/{model}_surface_std.nii.gz
    (float32).  The maps live on the contours of the fixed structures: NaN everywhere else, and in the std map where a contour
    voxel has fewer than two samples, written as NaN so that a viewer shows the surfaces alone."""
    folder = _folder(save_dirs, 'samples')
    for name, im in (('surface_bias', bias), ('surface_std', std)):
        logger.info(f'{model}_{name}: {int(np.isfinite(_np(im)).sum())} contour voxels hold a value, NaN elsewhere')
        save_im_to_disk(im, path.join(folder, f'{model}_{name}.nii.gz'), spacing)
