"""Trainer: the MCMC half of the reference's trainer/trainer.py, driving the fused HIP transition.

Kept surface (same names, arguments and return values as the reference):
  `Trainer(config, data_loader, losses, transformation_module, registration_module, metrics)`, `.run()`,
  `_SGLD_transition(fixed, moving, data_loss, reg_loss) -> (loss_terms, output, aux)`  (trainer.py:291-356),
  `step(...)` (alias asked for by BASELINE.json), `_run_MCMC` (:358-476), `_step_GMM` (:68-77).
The VI stage (`_run_VI`, `_test_VI`, trainer/vi.py) is composed in torch from the HIP-backed modules, as the reference
composes it; it hands its hyper-parameters and optimiser moments to the fused engine before the MCMC stage.

Inside `_SGLD_transition` nothing runs in torch: one call into the C ABI launches the whole transition on the current
HIP stream (ir_sgmcmc_amd/csrc/api_ctx.hip: transition_impl).  The hyper-parameters of the loss objects are mirrored into
the device state once (`_engine_init`) and read back lazily (`sync_parameters`) when something logs them.
"""
import dataclasses
import math
import os
import time
from collections import namedtuple

import numpy as np
import torch

from ..base import BaseTrainer
from .. import ops
from ..diagnostics import (COMPARISON_METRICS, COVARIANCE_METRICS, ChainMoments, DisplacementCovariance, DisplacementModes,
                           DisplacementQuantiles, ICE_SPACES, MODES_METRICS, displacement_modes_options,
                           IMAGE_METRICS, IMAGE_STD_FLOOR_FRACTION, IMAGE_Z_METRICS, ImagePosterior, image_posterior_names,
                           image_posterior_options, InverseConsistency, JACOBIAN_METRICS, JacobianPosterior, LABEL_STRUCTURE_METRICS, LANDMARK_METRICS,
                           LOCAL_METRICS, LabelPosterior, LandmarkPair, LandmarkPosterior, LocalSimilarity, QUANTILE_METRICS,
                           SURFACE_METRICS, SurfacePosterior, surface_coverage_key, surface_posterior_options,
                           diagnostics_period, displacement_covariance_options, displacement_quantiles_options,
                           ess_options, hausdorff_options, image_similarity_options, inverse_consistency_options, is_recorded,
                           jacobian_posterior_options, label_posterior_options, landmark_options, local_similarity_options,
                           NATIVE_POSTERIOR_IMAGE_METRICS, NativePosterior, native_posterior_options,
                           native_resolution_options, PosteriorComparison, posterior_comparison_options, ResidualCheck,
                           residual_check_options, residual_metrics,
                           SIMILARITY_METRICS, StructureReport, TruthCalibration, recorded_steps, voxel_scale)
from ..engine import EngineConfig, TransitionEngine, diff_op_code
from ..logger import (save_displacement_covariance, save_displacement_mean_and_std_dev, save_displacement_modes, save_displacement_quantiles, save_ess,
                      save_field, save_image_posterior, save_inverse_consistency, save_jacobian_posterior, save_label_posterior, save_landmarks,
                      save_local_similarity_of_mean, save_local_similarity_posterior, save_native_mean, save_native_posterior, save_native_sample,
                      save_posterior_comparison, save_precond_sigma,
                      save_residual_histogram, save_residual_nll, save_rhat, save_sample, save_structure_report, save_surface_posterior,
                      save_truth_calibration)
from .. import affine, bspline, image_posterior, mi, multires, ngf, preconditioner, residual_check, sghmc, structure_report
from .. import truth as truth_ops
from .. import masks as mask_ops  # (`masks` names the pair of masks in several methods below)
from ..multires import coarse_start_options
from ..utils import (calc_DSC_GPU, calc_image_similarity, calc_norm, calc_no_non_diffeomorphic_voxels, calc_residual_check,
                     init_identity_grid_3D, local_similarity_rows, sample_q_v, transform_coordinates)
from .vi import VIMixin


# A posterior recorder of the MCMC stage (Trainer._recorders): its checkpoint key, its state object (diagnostics.py), its
# period, the trainer.<option> that switches it on, the noun of the resume error, what it records of a transition (an
# output: 'displacement', 'transformation'; 'seg_warped': the warped moving segmentation; 'velocity': the dense velocity the
# exponential integrated; 'lncc': the LNCC maps of the warped moving image; 'residuals': the dense residuals of the data term;
# or a tuple of these, recorded as a tuple), its
# _finish_* method and what that takes first ('fixed': the fixed image's dict, 'moving_mask': the mask of the displacement std
# map, 'masks': {'fixed': ..., 'moving': ...})
Recorder = namedtuple('Recorder', 'key state period option noun records finish takes')


def mi_refusals(virtual_decimation, residual_options, vi):
    """what a run with the MI data loss cannot be combined with, each refused with its reason"""
    if virtual_decimation:
        raise ValueError('the MI data loss takes no virtual decimation (it has no residual whose correlation could be estimated): set '
                         '"virtual_decimation" to false')
    if residual_options is not None:
        raise ValueError('trainer.residual_check compares the residuals with the Gaussian mixture: it needs the GMM data loss, not MI')
    if vi:
        raise ValueError('the VI stage composes data_loss.map and data_loss.reduce, and MI is no per-voxel map followed by a masked sum: '
                         'set trainer."VI" to false with the MI data loss')


def ngf_refusals(virtual_decimation, residual_options):
    """what a run with the NGF data loss cannot be combined with, each refused with its reason"""
    if virtual_decimation:
        raise ValueError('the NGF data loss takes no virtual decimation (its map is no residual whose correlation could be estimated): '
                         'set "virtual_decimation" to false')
    if residual_options is not None:
        raise ValueError('trainer.residual_check compares the residuals with the Gaussian mixture: it needs the GMM data loss, not NGF')


ENGINE_DATA_LOSSES = ('GMM', 'SSD', 'LNCC', 'MI', 'NGF')


def engine_data_loss(kind):
    """the EngineConfig.data_loss of a data-loss class name; a class the fused transition does not know is refused (it used to run
    as SSD, silently)"""
    if kind not in ENGINE_DATA_LOSSES:
        raise ValueError(f'data_loss.type {kind!r} is not wired into the fused transition: one of {list(ENGINE_DATA_LOSSES)}')
    return kind


class LazyScalar:
    """a per-chain scalar that lives on the device until somebody calls .item() / float() on it (no sync otherwise)"""

    def __init__(self, fetch, key, idx):
        self._fetch, self._key, self._idx = fetch, key, idx

    def item(self):
        return float(self._fetch()[self._key][self._idx])

    __float__ = item

    def __add__(self, other):
        return self.item() + float(other)

    __radd__ = __add__

    def __repr__(self):
        return f'{self.item():.6g}'


class Trainer(VIMixin, BaseTrainer):
    def __init__(self, config, data_loader, losses, transformation_module, registration_module, metrics, device='cuda:0'):
        super().__init__(config, data_loader, losses, transformation_module, registration_module, metrics, device)
        self.Sobolev_grad = config['Sobolev_grad']['enabled']
        self.Sobolev_s = int(config['Sobolev_grad']['s']) if self.Sobolev_grad else 0
        self.Sobolev_lambda = float(config['Sobolev_grad']['lambda']) if self.Sobolev_grad else 0.0
        cfg_trainer = config['trainer']
        self.add_noise_uniform = cfg_trainer['uniform_noise']['enabled']
        self.alpha = cfg_trainer['uniform_noise']['magnitude'] if self.add_noise_uniform else 0.0
        self.virutal_decimation = config['virtual_decimation']  # (sic) reference attribute name, trainer.py:42
        self.engine = None
        self.v_curr_state, self.SGLD_params = None, None
        self._scalars_cache, self._outputs = None, None
        # affine pre-alignment of the pair before anything else sees it (affine.py, _affine_init): None when
        # trainer.affine_init is absent.  Read first: it refuses trainer.native_resolution and trainer.landmarks beside it
        self.affine_options = affine.affine_init_options(cfg_trainer, config['data_loader']['args']['dims'])
        self.affine_summary = None
        # automatic foreground masks (masks.py, _auto_mask): None when trainer.auto_mask is absent, and then nothing changes.
        # Computed from the pair on the registration grid before the pre-alignment; a resumed run computes them again
        self.auto_mask_options = mask_ops.auto_mask_options(cfg_trainer)
        self.auto_mask_summary = None
        if self.auto_mask_options is not None and self.auto_mask_options['source'] == 'file' and not getattr(data_loader, 'has_masks', True):
            raise ValueError('trainer.auto_mask: "source": "file" needs mask files, and the data loader found no "masks" directory')
        if (self.auto_mask_options is not None and self.auto_mask_options['source'] == 'image' and cfg_trainer.get('native_resolution')
                and not getattr(data_loader, 'has_masks', True)):
            raise ValueError('trainer.auto_mask with "source": "image" and no mask files cannot be combined with '
                             'trainer.native_resolution, which reads its masks on the native grid from files (masks on the native '
                             'grid are not computed)')
        # split-R-hat of the displacement (diagnostics.py): None when trainer.convergence_diagnostics is off
        self.diagnostics_period = diagnostics_period(cfg_trainer)
        self._chain_moments = None
        self.rhat, self.rhat_summary = None, None
        # split ESS / MCSE on top of it: None when its "ess" key is off
        self.ess_options = ess_options(cfg_trainer)
        self.ess, self.mcse, self.ess_summary = None, None, None
        # posterior label maps of the propagated segmentation (diagnostics.LabelPosterior): None when trainer.label_posterior
        # is off
        self.label_options = label_posterior_options(cfg_trainer)
        self._label_posterior = None
        self.label_entropy, self.label_map, self.label_summary = None, None, None
        # surface posterior of the propagated segmentation (diagnostics.SurfacePosterior): None when trainer.surface_posterior
        # is off
        self.surface_options = surface_posterior_options(cfg_trainer)
        self._surface_posterior = None
        self.surface_bias, self.surface_std, self.surface_summary = None, None, None
        # Jacobian posterior maps (diagnostics.JacobianPosterior): None when trainer.jacobian_posterior is off
        self.jacobian_options = jacobian_posterior_options(cfg_trainer)
        self._jacobian_posterior = None
        self.jacobian_fold_prob, self.jacobian_logJ_mean, self.jacobian_logJ_std, self.jacobian_summary = None, None, None, None
        # displacement covariance (diagnostics.DisplacementCovariance): None when trainer.displacement_covariance is off
        self.covariance_options = displacement_covariance_options(cfg_trainer)
        self._displacement_covariance = None
        self.displacement_cov_std, self.displacement_cov_direction = None, None
        self.displacement_cov_anisotropy, self.displacement_cov_summary = None, None
        # posterior principal modes (diagnostics.DisplacementModes): None when trainer.displacement_modes is off
        self.modes_options = displacement_modes_options(cfg_trainer)
        self._displacement_modes = None
        self.displacement_modes_summary, self.displacement_mode_fields, self.displacement_mode_scores = None, None, None
        # displacement credible intervals (diagnostics.DisplacementQuantiles): None when trainer.displacement_quantiles is off
        self.quantiles_options = displacement_quantiles_options(cfg_trainer)
        self._displacement_quantiles = None
        self.displacement_quantiles, self.displacement_ci_width, self.displacement_quantiles_summary = None, None, None
        # Hausdorff and percentile surface distances next to every logged ASD: None when trainer.hausdorff is off
        self.hausdorff_options = hausdorff_options(cfg_trainer)
        # inverse transformation and inverse-consistency error maps (diagnostics.InverseConsistency): None when
        # trainer.inverse_consistency is off
        self.ice_options = inverse_consistency_options(cfg_trainer)
        self._inverse_consistency = None
        self.ice_summary = None
        # outputs on the image's own voxel grid (ops.native_warp): None when trainer.native_resolution is off.  No state: the
        # native volumes go to the device in _run_MCMC
        self.native_options = native_resolution_options(cfg_trainer, data_loader)
        self._native = None
        # the label and the image posterior on the image's own voxel grid (native_posterior.py, diagnostics.NativePosterior): None
        # when trainer.native_posterior is off.  It needs trainer.native_resolution, whose loader supplies the native pair
        self.native_posterior_options = native_posterior_options(cfg_trainer, data_loader)
        self._native_posterior, self._native_std_floor = None, None
        self.native_posterior_maps, self.native_posterior_summary = None, None
        # image posterior: the moving image and the extra volumes on its grid carried through every recorded transformation
        # (image_posterior.py, diagnostics.ImagePosterior): None when trainer.image_posterior is off.  _image_volumes: the
        # volumes on the registration grid, formed in _run_model once the pair is masked and pre-aligned (a resumed run forms
        # them again: only the state goes into a checkpoint)
        self.image_options = image_posterior_options(cfg_trainer)
        self._image_posterior, self._image_volumes, self._image_std_floor = None, None, None
        self.image_maps, self.image_summary = None, None
        if self.image_options is not None and self.image_options['volumes']:
            if self.native_options is not None:
                raise ValueError('trainer.image_posterior.volumes cannot be combined with trainer.native_resolution: the extra '
                                 'volumes are read on the registration grid only')
            for v in self.image_options['volumes']:
                if not os.path.isfile(v['path']):
                    raise FileNotFoundError(f'trainer.image_posterior.volumes: {v["name"]!r}: no file {v["path"]!r}')
        # label-free similarity of the fixed and the warped moving image (ops.image_similarity): None when
        # trainer.image_similarity is off.  No state but the two intensity ranges, taken from the pair
        self.similarity_options = image_similarity_options(cfg_trainer)
        self._similarity_ranges, self._similarity_warned = None, False
        self.similarity_summary = None
        # landmark propagation and target registration error (diagnostics.LandmarkPosterior): None when trainer.landmarks is off
        self.landmark_options = landmark_options(cfg_trainer, data_loader)
        self._landmarks, self._landmark_unit = None, None
        self.landmark_summary = None
        # local similarity maps of the fixed and the warped moving image and the posterior of the LNCC maps
        # (ops.local_similarity, diagnostics.LocalSimilarity): None when trainer.local_similarity is off
        self.local_options = local_similarity_options(cfg_trainer)
        self._local_similarity, self._local_ranges, self._local_warned = None, None, False
        self.local_lncc_mean, self.local_lncc_min, self.local_similarity_summary = None, None, None
        # residual model check: the residuals against the mixture that models them, and the per-voxel NLL map
        # (residual_check.py, diagnostics.ResidualCheck): None when trainer.residual_check is off
        self.residual_options = residual_check_options(cfg_trainer)
        self._residual_check, self._residual_range, self._residual_warned = None, None, False
        self.residual_nll_mean, self.residual_summary = None, None
        # VI against MCMC: the distances between the Gaussians fitted to the displacements of the two stages
        # (posterior_comparison.py, diagnostics.PosteriorComparison): None when trainer.posterior_comparison is off
        self.comparison_options = posterior_comparison_options(cfg_trainer)
        self._posterior_comparison = None
        self.comparison_shift, self.comparison_log_std_ratio, self.comparison_bures, self.comparison_jeffreys = None, None, None, None
        self.comparison_summary = None
        # structure report: per structure of the fixed segmentation, the posterior of its mean displacement and volume change and
        # the per-structure rows of the maps above (structure_report.py, diagnostics.StructureReport): None when
        # trainer.structure_report is off
        self.structure_options = structure_report.structure_report_options(cfg_trainer, data_loader, self.structures_dict)
        self._structure_report = None
        self.structure_summary = None
        # known-transformation validation (truth.py, diagnostics.TruthCalibration): None when trainer.truth is absent, and then
        # nothing changes.  _truth: the dense truth on the device, in voxels as the transition writes the displacement, made (and,
        # with "simulate", the moving triple replaced) in _run_model; a resumed run makes it again and checks its fingerprint
        self.truth_options = truth_ops.truth_options(cfg_trainer)
        self._truth, self._truth_floor, self._truth_initial, self._truth_calibration = None, None, None, None
        self.truth_error, self.truth_mahalanobis, self.truth_summary = None, None, None
        # coarse-to-fine start (multires.py, _coarse_start): None unless trainer.MCMC_init is "coarse"
        self.coarse_options = coarse_start_options(cfg_trainer, config['data_loader']['args']['dims'],
                                                   config['transformation_module']['type'])
        self.coarse_summary = None
        # adaptive pSGLD preconditioner (preconditioner.py, _adapt_preconditioner): None when trainer.adaptive_preconditioner is
        # absent, and then nothing changes.  _precond: the estimator's state while sigma is still adapted; _precond_frozen_at:
        # the transition after which sigma stays as it is
        self.precond_options = preconditioner.adaptive_preconditioner_options(cfg_trainer, self.no_iters_burn_in)
        self._precond, self._precond_grad, self._precond_frozen_at = None, None, None
        self.preconditioner_summary = None
        # the sampler (sghmc.py): None when trainer.sampler is absent or {"type": "SGLD"}, and then nothing changes.  With "SGHMC"
        # the engine owns the momentum (engine.momentum); sampler_summary: the options and the last kinetic temperature logged
        self.sampler_options = sghmc.sampler_options(cfg_trainer)
        self.sampler_summary = None
        extra = sghmc.extra_optimizer_keys(config['optimizer_SG_MCMC'])
        if extra:  # (once: they have never been read, and still are not)
            self.logger.warning(f'optimizer_SG_MCMC.args: {extra} are ignored -- the field update reads "lr" and nothing else')
        # cubic B-spline resampling of the images that are saved (bspline.py): None unless trainer.output_interpolation is
        # "cubic".  _spline_coeff: the coefficients of the moving image, formed when the engine is set up (a resumed run forms
        # them again: nothing goes into a checkpoint)
        self.interpolation_options = bspline.output_interpolation_options(cfg_trainer)
        self._spline_coeff = None
        # a diagnostic that needs segmentations refuses here, not in the middle of a run, when the data loader has none
        if not getattr(data_loader, 'has_segs', True):
            for name, opt in (('label_posterior', self.label_options), ('surface_posterior', self.surface_options)):
                if opt is not None:
                    raise ValueError(f'trainer.{name} needs the fixed and the moving segmentation, and the data loader '
                                     f'({type(data_loader).__name__}) found no "segs" directory')

    # ---------------------------------------------------------------- automatic foreground masks
    def _auto_mask(self, fixed, moving):
        """trainer.auto_mask: the masks of the chosen sides replaced in place -- "source": "image": mask_ops.foreground_mask of the
        image; "file": the file mask with holes filled, closed and dilated.  self.auto_mask_summary, the auto_mask/{side}/*
        metrics, one log line per side and, with save_outputs and the option's save, samples/auto_mask_{side}.nii.gz.
        Deterministic: a resumed run computes the same masks again."""
        opt = self.auto_mask_options
        have_files = getattr(self.data_loader, 'has_masks', True)
        sp = getattr(self.data_loader, 'im_spacing', None)
        spacing = torch.ones(3) if sp is None else sp
        self.auto_mask_summary = {}
        self.writer.set_step(0)
        for side, triple in (('fixed', fixed), ('moving', moving)):
            if side not in mask_ops.auto_mask_sides(opt):
                continue
            file_mask = triple['mask'].bool() if have_files else None
            start = time.perf_counter()
            mask, summary = mask_ops.auto_mask(triple['im'], file_mask, opt)
            summary['seconds'] = time.perf_counter() - start
            voxels = int(mask.sum())
            summary.update(source=opt['source'], voxels_final=voxels, fraction=voxels / summary['total'])
            for key in ('threshold', 'components'):
                if key in summary:
                    self.metrics.update(f'auto_mask/{side}/{key}', float(summary[key]))
            self.metrics.update(f'auto_mask/{side}/voxels', float(voxels))
            self.metrics.update(f'auto_mask/{side}/fraction', summary['fraction'])
            if file_mask is not None:
                both = int((mask & file_mask).sum())
                summary['dice_vs_file'] = 2.0 * both / max(voxels + int(file_mask.sum()), 1)
                self.metrics.update(f'auto_mask/{side}/dice_vs_file', summary['dice_vs_file'])
            self.auto_mask_summary[side] = summary
            self.logger.info(f'auto mask ({side}, from the {opt["source"]}): {voxels} voxels, {100 * summary["fraction"]:.2f} % of the '
                             f'volume' + (f', threshold {summary["threshold"]:.6g}, {summary["components"]} components'
                                          if 'threshold' in summary else '') +
                             (f', Dice against the file mask {summary["dice_vs_file"]:.4f}' if 'dice_vs_file' in summary else '') +
                             f', box {summary["bounding_box"]}, {summary["seconds"]:.3f} seconds')
            triple['mask'] = mask
            if self.config['trainer'].get('save_outputs', True) and opt['save']:
                from ..logger import save_im_to_disk
                folder = self.config.save_dirs['samples']
                folder.mkdir(parents=True, exist_ok=True)
                save_im_to_disk(mask[0, 0].to(torch.uint8), str(folder / f'auto_mask_{side}.nii.gz'), spacing)

    # ---------------------------------------------------------------- affine pre-alignment
    def _affine_init(self, fixed, moving):
        """trainer.affine_init: the rigid / affine map of the pair (affine.register on fixed['im'], moving['im'] over
        fixed['mask']) -> the moving triple resampled through it; self.affine_summary, the affine/* metrics, one log line per
        level and, with save_outputs, samples/affine.json.  Deterministic: a resumed run computes the same map again."""
        opt = self.affine_options
        dims = tuple(int(n) for n in fixed['im'].shape[2:])
        sp = getattr(self.data_loader, 'im_spacing', None)
        spacing = np.ones(3) if sp is None else np.asarray(torch.as_tensor(sp).cpu(), dtype=np.float64).reshape(3)
        model = affine.AffineModel(opt['model'], spacing)
        start = time.perf_counter()
        lin, shift, history = affine.register(fixed['im'], moving['im'], fixed['mask'], model, opt['levels'], opt['max_iters'],
                                              opt['tol'], opt['min_overlap'], log=self.logger.info)
        aligned = affine.resample_pair(moving, lin, shift)
        seconds = time.perf_counter() - start
        summary = {'model': opt['model'], 'dims': list(dims), 'spacing': spacing.tolist(), 'lin': lin.tolist(), 'shift': shift.tolist(),
                   'index_matrix': affine.index_matrix(lin, shift, dims).tolist(),
                   'normalised_matrix': affine.normalised_matrix(lin, shift, dims).tolist(),
                   'mm_matrix': affine.mm_matrix(lin, shift, dims, spacing).tolist(), 'history': history,
                   'SSD_before': history[-1]['mean_ssd_first'] if len(history) == 1 else None, 'SSD_after': history[-1]['mean_ssd_last'],
                   'overlap': history[-1]['overlap'], 'iterations': sum(h['iterations'] for h in history), 'seconds': seconds}
        if summary['SSD_before'] is None:  # with coarser levels the full grid starts from their map: the identity is measured here
            f, m = affine._standardise(fixed['im'], moving['im'], fixed['mask'].bool())
            before = affine.normal_equations(f, m, fixed['mask'], np.eye(3), np.zeros(3))
            summary['SSD_before'] = before['ssd'] / max(before['n'], 1)
        if 'seg' in fixed and 'seg' in moving and self.structures_dict:
            for name, seg in (('DSC_before', moving['seg']), ('DSC_after', aligned['seg'])):
                DSC = calc_DSC_GPU(1, fixed['seg'], seg, self.structures_dict)
                summary[name] = {structure: float(DSC[0][j]) for j, structure in enumerate(self.structures_dict)}
        self.affine_summary = summary
        self.writer.set_step(0)
        for key in ('SSD_before', 'SSD_after', 'overlap', 'iterations'):
            self.metrics.update(f'affine/{key}', float(summary[key]))
        self.logger.info(f'affine pre-alignment ({opt["model"]}): mean SSD {summary["SSD_before"]:.6g} -> {summary["SSD_after"]:.6g} in '
                         f'{summary["iterations"]} iterations, {seconds:.2f} seconds')
        if self.config['trainer'].get('save_outputs', True):
            import json
            folder = self.config.save_dirs['samples']
            folder.mkdir(parents=True, exist_ok=True)
            with open(folder / 'affine.json', 'w') as f:
                json.dump(summary, f, indent=2)
        return aligned

    def _save_total_mean(self, mean, spacing):
        """samples/MCMC_sample_mean_total.vtk: the posterior-mean displacement composed with the pre-alignment, in mm as the
        mean itself is saved.  A(x + u) - x is affine in u, so the mean composes exactly."""
        from ..logger import save_field_to_disk
        ident = init_identity_grid_3D(mean.shape[1:], self.device).permute(0, 4, 1, 2, 3)
        s = self.affine_summary
        _, total = affine.compose((ident + transform_coordinates(mean.unsqueeze(0))).contiguous(), s['lin'], s['shift'])
        self.displacement_mean_total = total[0]
        folder = self.config.save_dirs['samples']
        folder.mkdir(parents=True, exist_ok=True)
        save_field_to_disk(total[0] * spacing[0], str(folder / 'MCMC_sample_mean_total.vtk'), spacing)

    # ---------------------------------------------------------------- engine plumbing
    def _engine_config(self):
        cfg = self.config
        data_loss, reg_loss = self.losses['data']['loss'], self.losses['reg']['loss']
        dims = tuple(cfg['data_loader']['args']['dims'])
        t_args = dict(cfg['transformation_module'].get('args', {}))
        kind = type(data_loss).__name__
        ec = dict(dims=dims, no_chains=self.no_chains, cps=tuple(t_args['cps']) if cfg['transformation_module']['type'] == 'SVFFD_3D' else None,
                  no_steps=getattr(self.transformation_module, 'no_steps', 12), sobolev_s=self.Sobolev_s,
                  sobolev_lambda=self.Sobolev_lambda, lr=float(cfg['optimizer_SG_MCMC']['args']['lr']),
                  uniform_noise=float(self.alpha), virtual_decimation=bool(self.virutal_decimation),
                  data_loss=engine_data_loss(kind), seed=int(cfg['trainer'].get('seed', 0)))
        if cfg['optimizer_SG_MCMC']['type'] != 'SGD':
            raise NotImplementedError('the SG-MCMC field update is plain SGD (reference configs), got ' + cfg['optimizer_SG_MCMC']['type'])
        if kind == 'GMM':
            o = cfg['optimizer_GMM']['args']
            sp = self.losses['data']['scale_prior'].normal
            ec.update(gmm_components=data_loss.no_components, lcc_s=data_loss.s, gmm_lr_log_std=o['lr_log_std'],
                      gmm_lr_logits=o['lr_logits'], gmm_lr_decay=o['lr_decay'],
                      scale_prior=(float(sp.loc), float(sp.log_scale.exp())),
                      dirichlet_alpha=[float(x) for x in self.losses['data']['proportion_prior'].concentration])
        elif kind == 'LNCC':
            if self.virutal_decimation:
                raise ValueError('the LNCC data loss takes no virtual decimation (its map is no residual whose correlation could be '
                                 'estimated): set "virtual_decimation" to false')
            if self.residual_options is not None:
                raise ValueError('trainer.residual_check compares the residuals with the Gaussian mixture: it needs the GMM data loss, '
                                 'not LNCC')
            ec.update(lcc_s=data_loss.radius, lncc_weight=data_loss.weight, lncc_eps=data_loss.eps)
        elif kind == 'MI':
            mi_refusals(self.virutal_decimation, self.residual_options, self.VI)
            # (the ranges: the loss object's, else what _engine_init found on the pair it hands the chains; until then None, and an
            # engine built from this config waits for mi_set)
            found = getattr(self, '_mi_ranges', None) or (None, None)
            ec.update(mi_bins=data_loss.bins, mi_weight=data_loss.weight, mi_fixed_range=data_loss.fixed_range or found[0],
                      mi_moving_range=data_loss.moving_range or found[1])
        elif kind == 'NGF':
            ngf_refusals(self.virutal_decimation, self.residual_options)
            # (the edge parameters: the loss object's, else what _engine_init found on the pair it hands the chains; until then None,
            # and an engine built from this config waits for ngf_set)
            found = getattr(self, '_ngf_eps', None) or (None, None)
            ec.update(ngf_weight=data_loss.weight, ngf_fixed_eps=data_loss.fixed_eps or found[0],
                      ngf_moving_eps=data_loss.moving_eps or found[1])
        else:
            ec.update(ssd_sigma=data_loss.sigma)
        rname = type(reg_loss).__name__
        if rname not in ('RegLoss_L2', 'RegLoss_LogNormal', 'RegLoss_Student', 'RegLoss_LogNormal_L2'):
            raise NotImplementedError(rname + ' is not wired into the fused transition')
        ec.update(reg_loss=rname, reg_learnable=bool(reg_loss.learnable), diff_op=type(reg_loss.diff_op).__name__)
        diff_op_code(ec['diff_op'])  # (raises for an operator the fused transition does not have)
        if rname == 'RegLoss_L2':
            ec.update(w_reg=float(reg_loss.log_w_reg.exp()))
            if reg_loss.learnable:
                o = cfg['optimizer_reg']['args']
                ec.update(reg_lr=(o['lr_log_w_reg'], 0.0), reg_lr_decay=o['lr_decay'])
        elif rname == 'RegLoss_Student':
            ec.update(student=(float(reg_loss.a0), float(reg_loss.b0_twice)))
        elif rname == 'RegLoss_LogNormal_L2':
            ec.update(w_reg=float(reg_loss.gamma_distr.rate) * 2.0)
        else:
            ec.update(w_reg=float(reg_loss.w_reg))
            if reg_loss.learnable:
                o = cfg['optimizer_reg']['args']
                lp, sp = self.losses['reg']['loc_prior'], self.losses['reg']['scale_prior'].normal
                ec.update(reg_lr=(o['lr_loc'], o['lr_log_scale']), reg_lr_decay=o['lr_decay'], loc_prior_nu=float(lp.nu),
                          loc_prior_w_reg=float(lp.w_reg), reg_scale_prior=(float(sp.loc), float(sp.log_scale.exp())))
        if self.sampler_options is not None:
            ec.update(sampler=self.sampler_options['type'], sghmc_friction=self.sampler_options['friction'],
                      sghmc_temperature=self.sampler_options['temperature'])
        return EngineConfig(**ec)

    def _engine_init(self, fixed, moving):
        if type(self.losses['data']['loss']).__name__ == 'MI':
            # once, from the pair the chains get (after auto_mask, affine_init and truth): the fixed image under its mask, the moving
            # image over the whole volume
            self._mi_ranges = mi.mi_ranges(fixed['im'], moving['im'], fixed['mask'])
        data_loss = self.losses['data']['loss']
        if type(data_loss).__name__ == 'NGF':
            # once, from the pair the chains get (after auto_mask, affine_init and truth): the mean of |grad I| of the fixed image under
            # its mask and of the moving image under its own mask, where the pair has one.  The config's nulls stay null: the values
            # found are this pair's (`found_eps` of the loss object, so that the VI stage runs with the same two), formed again for
            # the next pair
            self._ngf_eps = ngf.ngf_edge_parameters(fixed['im'], moving['im'], fixed.get('mask'), moving.get('mask'))
            data_loss.found_eps = self._ngf_eps
        self.engine = TransitionEngine(self._engine_config(), self.device)
        if self.engine.cfg.data_loss == 'NGF':
            ec = self.engine.cfg
            self.logger.info(f'NGF data term: weight {ec.ngf_weight:g}, fixed eps {ec.ngf_fixed_eps:.6g}, moving eps {ec.ngf_moving_eps:.6g}')
        if self.engine.cfg.data_loss == 'MI':
            ec = self.engine.cfg
            self.logger.info(f'MI data term: {ec.mi_bins} bins, weight {ec.mi_weight:g}, fixed range [{ec.mi_fixed_range[0]:.6g}, '
                             f'{ec.mi_fixed_range[1]:.6g}], moving range [{ec.mi_moving_range[0]:.6g}, {ec.mi_moving_range[1]:.6g}]')
        if self.sampler_options is not None:
            opt = self.sampler_options
            self.sampler_summary = {'options': dict(opt), 'kinetic_temperature': None}
            self.logger.info(f'sampler: SGHMC, friction {opt["friction"]:g}, temperature {opt["temperature"]:g} (momentum on the '
                             f'velocity grid, noise persisted in v; the forward pass adds none)')
        self._fixed, self._moving = self.engine.prepare(fixed, moving)
        self._mask_idx = None
        self._set_hyper_parameters(self.engine)
        if self.interpolation_options is not None:
            self._spline_coeff = self._spline_prefilter(moving['im'], 'the moving image')

    def _spline_prefilter(self, im, what):
        """the cubic B-spline coefficients of `im` (.,1,D,H,W), with the one log line of trainer.output_interpolation"""
        torch.cuda.synchronize()
        start = time.perf_counter()
        coeff = bspline.prefilter(im.contiguous())
        peak = float(coeff.abs().max())  # the read-back waits for the three passes
        self.logger.info(f'output interpolation: cubic B-spline of {what} {tuple(im.shape[2:])}, max|c| {peak:.6g}, prefilter '
                         f'{time.perf_counter() - start:.4f} seconds')
        return coeff

    def _saved_image(self, im_moving_warped, transformation):
        """the warped moving image that goes to disk: the transition's trilinear one, or -- trainer.output_interpolation
        "cubic" -- the spline of the moving image at the same transformation.  The chain and every metric keep reading the
        trilinear image."""
        if self._spline_coeff is None:
            return im_moving_warped
        return bspline.warp(self._spline_coeff, transformation.contiguous())

    def _set_hyper_parameters(self, engine, lognormal=True):
        """hyper-parameters of the loss objects -> the device state of `engine`.  lognormal False leaves RegLoss_LogNormal's
        (loc, log_scale) as the engine initialised them for ITS grid (engine.lognormal_init): the loss object's loc was
        computed for the degrees of freedom of the full grid."""
        st = engine.state()
        data_loss, reg_loss = self.losses['data']['loss'], self.losses['reg']['loss']
        if type(data_loss).__name__ == 'GMM':
            for k in range(data_loss.no_components):
                st.gmm_log_std[k], st.gmm_logits[k] = float(data_loss.log_std[k].detach()), float(data_loss.logits[k].detach())
        if type(reg_loss).__name__ == 'RegLoss_L2':
            st.reg_param[0] = float(reg_loss.log_w_reg.detach())
        elif type(reg_loss).__name__ == 'RegLoss_LogNormal' and lognormal:
            st.reg_param[0], st.reg_param[1] = float(reg_loss.loc.detach()), float(reg_loss.log_scale.detach())
        engine.set_state(st)

    def sync_parameters(self):
        """device state -> the nn.Parameters of the loss objects (what the reference's logging reads, trainer.py:391-402)"""
        st = self.engine.state()
        data_loss, reg_loss = self.losses['data']['loss'], self.losses['reg']['loss']
        with torch.no_grad():
            if type(data_loss).__name__ == 'GMM':
                K = data_loss.no_components
                data_loss.log_std.copy_(torch.tensor(list(st.gmm_log_std)[:K]))
                data_loss.logits.copy_(torch.tensor(list(st.gmm_logits)[:K]))
            if type(reg_loss).__name__ == 'RegLoss_L2':
                reg_loss.log_w_reg.fill_(st.reg_param[0])
            elif type(reg_loss).__name__ == 'RegLoss_LogNormal':
                reg_loss.loc.fill_(st.reg_param[0])
                reg_loss.log_scale.fill_(st.reg_param[1])
        return st

    def _scalars(self):
        if self._scalars_cache is None:
            self._scalars_cache = self.engine.scalars()
        return self._scalars_cache

    def _recorders(self):
        """the active recorders, in the order they record and finish: moments, labels, surfaces, Jacobian, images, covariance,
        modes, quantiles, inverse consistency, landmarks, local similarity, residual check, posterior comparison, truth
        calibration, native posterior, and last the structure report, which reads the maps the others have finished"""
        period = lambda options: options and options['period']
        rows = (('chain_moments', self._chain_moments, self.diagnostics_period, 'convergence_diagnostics', 'chain moments',
                 'displacement', self._finish_diagnostics, 'moving_mask'),
                ('label_posterior', self._label_posterior, period(self.label_options), 'label_posterior', 'label posterior',
                 'seg_warped', self._finish_label_posterior, 'fixed'),
                ('surface_posterior', self._surface_posterior, period(self.surface_options), 'surface_posterior',
                 'surface posterior', 'seg_warped', self._finish_surface_posterior, 'fixed'),
                ('jacobian_posterior', self._jacobian_posterior, period(self.jacobian_options), 'jacobian_posterior',
                 'Jacobian posterior', 'transformation', self._finish_jacobian_posterior, 'fixed'),
                ('image_posterior', self._image_posterior, period(self.image_options), 'image_posterior', 'image posterior',
                 'transformation', self._finish_image_posterior, 'fixed'),
                ('displacement_covariance', self._displacement_covariance, period(self.covariance_options),
                 'displacement_covariance', 'displacement covariance', 'displacement', self._finish_displacement_covariance,
                 'moving_mask'),
                ('displacement_modes', self._displacement_modes, period(self.modes_options), 'displacement_modes',
                 'displacement modes', 'displacement', self._finish_displacement_modes, 'moving_mask'),
                ('displacement_quantiles', self._displacement_quantiles, period(self.quantiles_options), 'displacement_quantiles',
                 'displacement quantiles', 'displacement', self._finish_displacement_quantiles, 'moving_mask'),
                ('inverse_consistency', self._inverse_consistency, period(self.ice_options), 'inverse_consistency',
                 'inverse consistency', ('velocity', 'transformation', 'displacement'), self._finish_inverse_consistency, 'masks'),
                ('landmarks', self._landmarks, period(self.landmark_options), 'landmarks', 'landmark posterior',
                 ('displacement', 'velocity') if self.landmark_options and self.landmark_options['inverse'] else 'displacement',
                 self._finish_landmarks, 'masks'),
                ('local_similarity', self._local_similarity, period(self.local_options), 'local_similarity', 'local similarity',
                 'lncc', self._finish_local_similarity, 'fixed'),
                ('residual_check', self._residual_check, period(self.residual_options), 'residual_check', 'residual check',
                 'residuals', self._finish_residual_check, 'fixed'),
                ('posterior_comparison', self._posterior_comparison, period(self.comparison_options), 'posterior_comparison',
                 'posterior comparison', 'displacement', self._finish_posterior_comparison, 'moving_mask'),
                ('truth_calibration', self._truth_calibration, period(self.truth_options), 'truth', 'truth calibration',
                 'displacement', self._finish_truth_calibration, 'fixed'),
                ('native_posterior', self._native_posterior, period(self.native_posterior_options), 'native_posterior',
                 'native posterior', 'displacement', self._finish_native_posterior, 'fixed'),
                ('structure_report', self._structure_report, period(self.structure_options), 'structure_report',
                 'structure report', ('displacement', 'transformation'), self._finish_structure_report, 'fixed'))
        return [Recorder(*row) for row in rows if row[1] is not None]

    # ---------------------------------------------------------------- checkpoint / resume (absent in the reference)
    def state_dict(self):
        """Everything a chain needs to continue bit-for-bit: the velocity field, the SGLD pre-conditioner, the device-side
        hyper-parameter state (GMM / regulariser parameters, their Adam moments and step counts, the Philox iteration
        counter) and the running posterior moments."""
        import ctypes
        st = self.engine.state()
        sigma = getattr(self, '_sigma', None)
        return {'v_curr_state': self.v_curr_state.detach().cpu(), 'sigma': None if sigma is None else sigma.detach().cpu(),
                'tau': self.SGLD_params['tau'], 'engine_state': bytes(ctypes.string_at(ctypes.byref(st), ctypes.sizeof(st))),
                'sample_no': getattr(self, '_sample_no', 0),
                'moments': {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in getattr(self, '_moments', {}).items()},
                'config_name': self.config['name'],
                **({'preconditioner': preconditioner.checkpoint_entry(self._precond, self._precond_frozen_at)}
                   if self._precond is not None else {}),
                **({'momentum': self.engine.momentum.detach().cpu()} if self.engine.momentum is not None else {}),
                **{r.key: r.state.state_dict() for r in self._recorders()}}

    def load_state_dict(self, sd):
        import ctypes
        from .. import _lib as L
        if self.engine is None:
            raise RuntimeError('load_state_dict: call _engine_init(fixed, moving) first')
        st = L.IrsState()
        raw = sd['engine_state']
        if len(raw) != ctypes.sizeof(st):
            raise ValueError('checkpoint was written by an incompatible build (state struct size differs)')
        ctypes.memmove(ctypes.byref(st), raw, len(raw))
        self.engine.set_state(st)
        self.v_curr_state = sd['v_curr_state'].to(self.device).contiguous()
        self._sigma = None if sd['sigma'] is None else sd['sigma'].to(self.device).contiguous()
        self.SGLD_params = {'tau': sd['tau'], 'sigma': self._sigma if self._sigma is not None else torch.ones_like(self.v_curr_state)}
        self._sample_no = int(sd['sample_no'])
        self._moments = {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in sd.get('moments', {}).items()}
        if self.precond_options is not None:
            preconditioner.check_checkpoint(sd, self.precond_options, self._sample_no)
            self._precond_restore(sd.get('preconditioner'))
        if self.engine.momentum is not None:
            if 'momentum' in sd:
                self.engine.momentum.copy_(sd['momentum'].to(self.device))
            elif self._sample_no > 0:
                raise ValueError(f'the checkpoint at sample {self._sample_no} holds no momentum (written with trainer.sampler off or '
                                 f'"SGLD") but this run samples with SGHMC')
            else:
                self.engine.momentum.zero_()
        for r in self._recorders():
            if r.key in sd:
                r.state.load_state_dict(sd[r.key])
            elif any(is_recorded(s, self.no_iters_burn_in, r.period) for s in range(1, self._sample_no + 1)):
                raise ValueError(f'the checkpoint at sample {self._sample_no} holds no {r.noun} (written with '
                                 f'trainer.{r.option} off) but this run records from sample '
                                 f'{self.no_iters_burn_in + r.period} on')
        self.sync_parameters()

    def save_checkpoint(self, file_path):
        torch.save(self.state_dict(), file_path)

    def load_checkpoint(self, file_path):
        # plain tensors, numbers and bytes only: a checkpoint is data, never code
        self.load_state_dict(torch.load(file_path, map_location='cpu', weights_only=True))

    # ---------------------------------------------------------------- reference-named pieces
    def _SGLD_init(self, var_params_q_v):
        """Trainer.__SGLD_init (trainer.py:585-611)"""
        shape = [self.no_chains, 3, *var_params_q_v['mu'].shape[-3:]]
        if self.MCMC_init == 'VI':
            vp = {k: v.to(self.device).reshape(1, 3, *shape[2:]) for k, v in var_params_q_v.items()}
            v = torch.empty(shape, device=self.device)
            for idx in range(self.no_chains):
                v[idx] = sample_q_v(vp, no_samples=1)[0]
            sigma = torch.exp(0.5 * vp['log_var']).expand(shape).contiguous()
        elif self.MCMC_init == 'identity':
            v, sigma = torch.zeros(shape, device=self.device), None
        elif self.MCMC_init == 'noise':
            v, sigma = torch.randn(shape, device=self.device), None
        elif self.MCMC_init == 'coarse':
            if self.config['trainer'].get('resume'):  # the checkpoint supplies v
                self.logger.info('coarse start: skipped, the run resumes from a checkpoint')
                self.coarse_summary = []
                v, sigma = torch.zeros(shape, device=self.device), None
            else:
                v, sigma = self._coarse_start(), None
        else:
            raise ValueError(self.MCMC_init)
        tau = self.config['optimizer_SG_MCMC']['args']['lr']
        self.SGLD_params = {'sigma': sigma if sigma is not None else torch.ones(shape, device=self.device), 'tau': tau}
        self._sigma = sigma  # None = identity preconditioner (the kernels skip the load)
        self.v_curr_state = v.contiguous()
        C, dv, d = self.no_chains, tuple(shape[2:]), tuple(self.config['data_loader']['args']['dims'])
        new = lambda *s: torch.empty(*s, device=self.device, dtype=torch.float32)
        self._outputs = {'curr_state': new(C, 3, *dv), 'im_moving_warped': new(C, 1, *d), 'residuals': new(C, 1, *d),
                         'displacement': new(C, 3, *d), 'transformation': new(C, 3, *d)}

    def _coarse_start(self):
        """The start of MCMC_init "coarse": short chains on the pair restricted to every level of trainer.coarse_start, coarse
        to fine, each started from the prolonged result of the level below (zero at the first) -> v (no_chains,3,D,H,W) on the
        full grid.  Every level restricts from the FULL volumes, runs all chains in one engine of its own (identity
        pre-conditioner, in-kernel noise, seed + 1 + level) and is dropped before the next one allocates; the mixture of the
        run's engine is then re-seeded from the residuals of the prolonged field (nothing to do for an SSD).  Fills
        self.coarse_summary, one entry per level."""
        dims = tuple(self.config['data_loader']['args']['dims'])
        base = self._engine_config()
        self.coarse_summary = []
        v = None
        for no, level in enumerate(self.coarse_options['levels']):
            torch.cuda.synchronize(self.device)
            start = time.perf_counter()
            d, lr = level['dims'], base.lr if level['lr'] is None else level['lr']
            # (the levels keep the reference's update whatever trainer.sampler says: their job is a start, not samples)
            engine = TransitionEngine(dataclasses.replace(base, dims=d, lr=lr, seed=base.seed + 1 + no, sampler='SGLD'), self.device)
            fixed, moving = engine.prepare(*multires.restrict_pair(self._fixed, self._moving, d))
            self._set_hyper_parameters(engine, lognormal=False)
            v = torch.zeros((self.no_chains, 3, *d), device=self.device) if v is None else multires.prolong_field(v, d)
            engine.gmm_init(fixed, moving, None if no == 0 else v[:1])
            first = None
            for it in range(level['no_iters']):
                engine.transition(fixed, moving, v)
                if it == 0:
                    first = engine.scalars()['data_term']
            engine.flush()
            last = engine.scalars()['data_term']
            del engine, fixed, moving
            torch.cuda.synchronize(self.device)
            entry = {'dims': d, 'no_iters': level['no_iters'], 'lr': lr, 'data_term_first': first, 'data_term_last': last,
                     'seconds': time.perf_counter() - start}
            self.coarse_summary.append(entry)
            self.logger.info(f'coarse start, level {no}: dims {list(d)}, {entry["no_iters"]} transitions at lr {lr:g} in '
                             f'{entry["seconds"]:.2f} s; data term per chain {[f"{x:.6g}" for x in first]} -> '
                             f'{[f"{x:.6g}" for x in last]}')
        v = multires.prolong_field(v, dims)
        self.engine.gmm_init(self._fixed, self._moving, v[:1])
        self.sync_parameters()
        return v

    # ---------------------------------------------------------------- adaptive pSGLD preconditioner (absent in the reference)
    def _precond_init(self):
        """the estimator of trainer.adaptive_preconditioner at the start of a run: a zero second moment on the velocity grid.
        self._sigma stays as _SGLD_init left it (None) until the first refresh: up to then the chain is the sigma-free chain"""
        self._precond = preconditioner.preconditioner_state(self.v_curr_state.shape, self.device)
        self._precond_grad, self._precond_frozen_at = None, None
        self.preconditioner_summary = {'options': dict(self.precond_options), 'refreshes': [], 'frozen_at': None}

    def _precond_restore(self, entry):
        """the estimator as a checkpoint holds it (entry None: a checkpoint past `until` written without the option -- its sigma
        is the frozen field, and nothing more is adapted)"""
        if entry is None:
            self._precond, frozen = None, self.precond_options['until']
        else:
            self._precond = {'V': entry['V'].to(self.device).contiguous(), 'count': int(entry['count']),
                             'nonfinite': torch.tensor([int(entry['nonfinite'])], device=self.device, dtype=torch.int64)}
            frozen = None if int(entry['frozen']) < 0 else int(entry['frozen'])
        self._precond_frozen_at = frozen
        if self.preconditioner_summary is None:
            self.preconditioner_summary = {'options': dict(self.precond_options), 'refreshes': [], 'frozen_at': None}
        self.preconditioner_summary['frozen_at'] = frozen  # the refreshes of a resumed run are those it made itself

    def _adapt_preconditioner(self, step, mask, spacing):
        """After adapting transition `step` (<= until): its gradient into the second moment, and at a refresh the new sigma.
        grad_v belongs to transition `step` only once nothing is pending, hence the flush -- one host synchronisation per
        adapting transition, none afterwards."""
        opt = self.precond_options
        self.engine.flush()
        preconditioner.preconditioner_accumulate(self._precond_grad, self._sigma, self._precond, opt['beta'])
        if not preconditioner.is_refresh(step, opt):
            return
        sigma, summary = preconditioner.preconditioner_sigma(self._precond, self.no_chains, opt['beta'], opt['smooth'], opt['damping'],
                                                             opt['sigma_min'], opt['sigma_max'])
        if summary['nonfinite']:
            raise RuntimeError(f'adaptive preconditioner: {summary["nonfinite"]} non-finite gradient values up to transition {step} '
                               f'(a chain has diverged; lower the learning rate or sigma_max)')
        self._sigma = sigma
        self.SGLD_params['sigma'] = sigma
        for key in preconditioner.METRICS:
            self.metrics.update(f'MCMC/precond/{key}', summary[key])
        self.preconditioner_summary['refreshes'].append({'step': step, **summary})
        self.logger.info(f'adaptive preconditioner, transition {step}: sigma in [{summary["sigma_min"]:.4g}, {summary["sigma_max"]:.4g}], '
                         f'mean sigma^2 {summary["sigma2_mean"]:.4g}, clamped {summary["clamped_low"]} low / {summary["clamped_high"]} high')
        if step == opt['until']:
            self._precond_frozen_at = self.preconditioner_summary['frozen_at'] = step
            self._precond_grad = None
            self.logger.info(f'adaptive preconditioner: sigma frozen after transition {step}')
            if opt['save'] and self.config['trainer'].get('save_outputs', True) and self.config['transformation_module']['type'] == 'SVF_3D':
                rms = sigma[0].square().mean(dim=0).sqrt()
                save_precond_sigma(self.logger, self.config.save_dirs, spacing, rms, mask)

    def _GMM_init(self, fixed, moving, var_params_q_v=None):
        """Trainer.__GMM_init (trainer.py:529-547): one velocity sample, std of the masked residual, 25 warm-up steps"""
        # the reference draws sample_q_v(var_params_q_v) here whatever MCMC_init is (mu = 0, sigma_v_init, u_v_init at the
        # start of a run): the residual std -- and with it the mixture's initial log_std and warm-up trajectory -- comes
        # from THAT warp, not from the identity
        v_sample = None
        if var_params_q_v is not None:
            vp = {k: v.to(self.device).reshape(1, 3, *v.shape[-3:]) for k, v in var_params_q_v.items()}
            v_sample = sample_q_v(vp).contiguous()
        self.engine.gmm_init(self._fixed, self._moving, v_sample)
        self.sync_parameters()

    def _SGLD_transition(self, fixed, moving, data_loss=None, reg_loss=None, eps=None, unif=None, with_outputs=True,
                         like_reference=True):
        """One SG-MCMC transition (trainer.py:291-356).  Returns (loss_terms, output, aux) with the reference's keys.

        `eps` / `unif` inject the two noise draws (parity runs); by default they come from in-kernel Philox.
        `like_reference` (default): `output[...]` are CLONES (trainer.py:302-305) and `aux['residuals']` is the masked view
        `residuals[fixed['mask']].view(no_chains, -1)` (trainer.py:308) -- a caller that keeps samples or feeds the residuals
        to its own code sees exactly the reference's objects.  With False the tensors are the engine-owned buffers the NEXT
        transition overwrites and the residuals stay dense (C,1,D,H,W): what this package's own `_run_MCMC` loop uses, since
        it consumes them at once (saves four volume copies and a gather per transition).
        """
        if self.engine is None:
            raise RuntimeError('call _engine_init / _run_MCMC first')
        out = self._outputs if with_outputs else {k: self._outputs[k] for k in ('curr_state', 'im_moving_warped', 'residuals')}
        if self._precond_grad is not None:  # an adapting transition of the adaptive preconditioner: it reads the gradient
            out = {**out, 'grad_v': self._precond_grad}
        self.engine.transition(self._fixed, self._moving, self.v_curr_state, self._sigma, eps, unif, out)
        self._scalars_cache = None
        C = self.no_chains
        lazy = lambda key: [LazyScalar(self._scalars, key, i) for i in range(C)]
        loss_terms = {'data': lazy('data_term'), 'reg': lazy('reg_term')}
        output = {'im_moving_warped': self._outputs['im_moving_warped'], 'displacement': self._outputs['displacement'],
                  'transformation': self._outputs['transformation'], 'curr_state': self._outputs['curr_state']}
        residuals = self._outputs['residuals']
        if like_reference:
            output = {k: v.clone() for k, v in output.items()}
            residuals = residuals.reshape(-1).index_select(0, self._masked_index()).view(C, -1)
        aux = {'residuals': residuals, 'alpha': lazy('alpha'), 'reg_energy': lazy('reg_energy')}
        return loss_terms, output, aux

    def _masked_index(self):
        """flat indices of the masked voxels of all chains, computed once (a boolean index would synchronise every transition)"""
        if getattr(self, '_mask_idx', None) is None:
            m = self._fixed['mask']
            m = m.expand(self.no_chains, *m.shape[1:]) if m.shape[0] == 1 else m
            self._mask_idx = m.reshape(-1).nonzero(as_tuple=False).squeeze(1)
        return self._mask_idx

    step = _SGLD_transition  # BASELINE.json calls the iteration `step()`

    # ---------------------------------------------------------------- MCMC driver (trainer.py:358-476)
    def _run_MCMC(self, fixed, moving, var_params_q_v):
        data_loss, reg_loss = self.losses['data']['loss'], self.losses['reg']['loss']
        self._SGLD_init(var_params_q_v)
        log = self.logger.info
        log(f'\nNO. CHAINS: {self.no_chains}, BURNING IN...')
        n_total = self.no_iters_burn_in + self.no_samples_MCMC
        # the reference logs hyper-parameters and loss terms on every iteration of a short run (trainer.py:389), each a host
        # read-back; `trainer.metrics_period` > 1 thins them out (the device then runs ahead of the host between reads)
        every = int(self.config['trainer'].get('metrics_period', 1 if self.no_samples_MCMC < 1e4 else 100))
        # running posterior mean / M2 of the displacement on the device instead of a
        # host array of every logged sample (trainer.py:365-366)
        mean = torch.zeros_like(self._outputs['displacement'][0])
        m2 = torch.zeros_like(mean)
        n_rec = 0
        cfg_trainer = self.config['trainer']
        checkpoint_period, save_samples = int(cfg_trainer.get('checkpoint_period', 0)), bool(cfg_trainer.get('save_samples', False))
        spacing = self.data_loader.im_spacing if getattr(self.data_loader, 'im_spacing', None) is not None else torch.ones(3)
        first = 1
        if self.diagnostics_period is not None:
            self._chain_moments = ChainMoments(self.no_chains, self._outputs['displacement'].shape[2:],
                                               self.no_samples_MCMC // self.diagnostics_period, self.device,
                                               max_lag=self.ess_options['max_lag'] if self.ess_options else None)
        if self.label_options is not None:
            if 'seg' not in fixed or 'seg' not in moving:
                raise ValueError('trainer.label_posterior needs the fixed and the moving segmentation ("seg" in both); '
                                 f'fixed has {sorted(fixed)}, moving has {sorted(moving)}')
            self._label_posterior = LabelPosterior(self.structures_dict, self._outputs['displacement'].shape[2:], self.device)
        if self.surface_options is not None:
            if 'seg' not in fixed or 'seg' not in moving:
                raise ValueError('trainer.surface_posterior needs the fixed and the moving segmentation ("seg" in both); '
                                 f'fixed has {sorted(fixed)}, moving has {sorted(moving)}')
            self._surface_posterior = SurfacePosterior(fixed['seg'][:1], self.structures_dict, spacing, self.device)
        if self.jacobian_options is not None:
            self._jacobian_posterior = JacobianPosterior(self._outputs['transformation'].shape[2:], self.device)
        if self.image_options is not None:
            if self._image_volumes is None:
                self._image_init(fixed, moving)
            self._image_posterior = ImagePosterior(self._image_volumes, image_posterior_names(self.image_options), self.device)
        if self.covariance_options is not None:
            self._displacement_covariance = DisplacementCovariance(self._outputs['displacement'].shape[2:], self.device)
        if self.quantiles_options is not None:
            q = self.quantiles_options
            self._displacement_quantiles = DisplacementQuantiles(self._outputs['displacement'].shape[2:], self.device, q['bins'],
                                                                 q['bin_width'])
            self.logger.info(f'displacement quantiles: {q["bins"]} bins of {q["bin_width"]:g} voxels, '
                             f'{self._displacement_quantiles.bytes_per_voxel(q["bins"])} bytes per voxel, '
                             f'{self._displacement_quantiles.state_bytes() / 1e6:.1f} MB on the device')
        masks = {'fixed': fixed['mask'][0], 'moving': moving.get('mask', fixed['mask'])[0]}
        if self.modes_options is not None:  # its mask, the std map's, is fixed here: it enters the Gram matrix
            self._displacement_modes = DisplacementModes(self._outputs['displacement'].shape[2:], self.device,
                                                         self.modes_options['max_records'], masks['moving'], self.logger)
        if self.ice_options is not None:
            self._inverse_consistency = InverseConsistency(self._outputs['displacement'].shape[2:], self.device,
                                                           getattr(self.transformation_module, 'no_steps', 12), masks)
        ice_dice = (self.ice_options is not None and self.ice_options['moving_space_dice'] and 'seg' in moving and 'seg' in fixed
                    and bool(self.structures_dict))
        if self.native_options is not None:
            self._native_init()
        if self.native_posterior_options is not None:
            self._native_posterior_init()
        if self.similarity_options is not None:
            self._similarity_init(fixed, moving)
        if self.landmark_options is not None:
            self._landmarks_init(self._outputs['displacement'].shape[2:])
        if self.local_options is not None:
            self._local_init(fixed, moving)
            self._local_similarity = LocalSimilarity(self._outputs['displacement'].shape[2:], self.device)
        if self.residual_options is not None:
            self._residual_init(fixed, moving)
            self._residual_check = ResidualCheck(self._outputs['residuals'].shape[2:], self.no_chains, self.device,
                                                 self._residual_range, self.residual_options['bins'], fixed['mask'][:1],
                                                 self.residual_options['nll_map'])
        if self.comparison_options is not None:
            self._comparison_init(self._outputs['displacement'].shape[2:])
        if self.precond_options is not None:
            self._precond_init()
        if self.truth_options is not None:
            self._truth_calibration_init(masks['fixed'])
        if self.structure_options is not None:
            if 'seg' not in fixed:
                raise ValueError(f'trainer.structure_report needs the fixed segmentation ("seg"); fixed has {sorted(fixed)}')
            # scale (1, 1, 1): voxels of the registration grid, the unit of the displacement covariance; no mask: the structures
            # are the regions
            steps = self.no_samples_MCMC // self.structure_options['period']
            self._structure_report = StructureReport(fixed['seg'][0], self.structures_dict, steps * self.no_chains, self.device)
        if cfg_trainer.get('resume'):
            self.load_checkpoint(cfg_trainer['resume'])
            first = self._sample_no + 1
            if self._moments:
                mean, m2, n_rec = self._moments['mean'], self._moments['m2'], int(self._moments['n'])
            log(f'resumed from {cfg_trainer["resume"]} at sample {self._sample_no}')
        recorders = self._recorders()
        for sample_no in range(first, n_total + 1):
            if sample_no < self.no_iters_burn_in and sample_no % self.log_period_MCMC == 0:
                log(f'burn-in sample no. {sample_no}/{self.no_iters_burn_in}')
            adapting = self.precond_options is not None and sample_no <= self.precond_options['until']
            if adapting and self._precond_grad is None:
                self._precond_grad = torch.empty_like(self.v_curr_state)
            loss_terms, output, aux = self._SGLD_transition(fixed, moving, data_loss, reg_loss, like_reference=False)
            if adapting:
                self._adapt_preconditioner(sample_no, masks['moving'], spacing)
            if sample_no == self.no_iters_burn_in:
                log('ENDED BURNING IN')
            seg_warped = None  # the warped segmentation of this step, when the Dice / ASD branch builds it
            lncc = None  # the LNCC maps of this step, when the logging branch forms them
            logged = False  # a step whose sample is logged (and, with save_samples, saved)
            self.writer.set_step(sample_no)
            if (sample_no - 1) % every == 0:
                st = self.sync_parameters()
                if type(data_loss).__name__ == 'GMM':
                    for idx in range(data_loss.no_components):
                        self.metrics.update(f'MCMC/GMM/scale_{idx}', data_loss.scales[idx].item())
                        self.metrics.update(f'MCMC/GMM/proportion_{idx}', data_loss.proportions[idx].item())
                if getattr(reg_loss, 'learnable', False):  # trainer.py:397-402
                    if type(reg_loss).__name__ == 'RegLoss_LogNormal':
                        self.metrics.update('MCMC/reg/loc', reg_loss.loc.item())
                        self.metrics.update('MCMC/reg/scale', reg_loss.scale.item())
                    elif type(reg_loss).__name__ == 'RegLoss_L2':
                        self.metrics.update('MCMC/reg/w_reg', reg_loss.log_w_reg.exp().item())
                total = sum(t.item() for t in loss_terms['data']) + sum(t.item() for t in loss_terms['reg'])
                self.metrics.update('MCMC/avg_loss', total / self.no_chains)
                for idx in range(self.no_chains):
                    self.metrics.update(f'MCMC/chain_{idx}/data_term', loss_terms['data'][idx].item())
                    self.metrics.update(f'MCMC/chain_{idx}/reg_term', loss_terms['reg'][idx].item())
                    self.metrics.update(f'MCMC/chain_{idx}/VD/alpha', aux['alpha'][idx].item())
                    self.metrics.update(f'MCMC/chain_{idx}/reg/energy', aux['reg_energy'][idx].item())
            if sample_no > self.no_iters_burn_in and (sample_no % self.log_period_MCMC == 0 or sample_no == self.no_samples_MCMC):
                # The outputs of a call are only those of sample `sample_no` once nothing is pending: a transition dropped by a failed
                # kernel-variant prediction is re-run by a LATER call, and until then the output buffers hold an earlier sample
                # (one sync per log_period; normally a no-op)
                self.engine.flush()
                logged = True
                transformation, displacement = output['transformation'], output['displacement']
                no_folds, log_det_J = calc_no_non_diffeomorphic_voxels(transformation, self.diff_op)
                if 'seg' in moving and 'seg' in fixed and self.structures_dict:
                    seg_warped = self.registration_module(moving['seg'], transformation)
                    self._log_segmentation_metrics([f'MCMC/chain_{idx}' for idx in range(self.no_chains)], fixed['seg'], seg_warped,
                                                   spacing)
                no_voxels = int(np.prod(displacement.shape[2:]))
                if save_samples:
                    saved_im = self._saved_image(output['im_moving_warped'], transformation)
                    for idx in range(self.no_chains):
                        save_sample(self.config.save_dirs, spacing, sample_no, saved_im[idx:idx + 1],
                                    displacement[idx:idx + 1], log_det_J[idx:idx + 1], 'MCMC', chain_no=idx)
                if self.sampler_options is not None:
                    kt = sghmc.kinetic_temperature(self.engine.momentum, self._sigma, self.engine.cfg.lr,
                                                   self.sampler_options['friction']).tolist()
                    self.sampler_summary['kinetic_temperature'] = kt
                    for idx in range(self.no_chains):
                        self.metrics.update(f'MCMC/chain_{idx}/sampler/kinetic_temperature', kt[idx])
                for idx in range(self.no_chains):
                    n_rec += 1
                    delta = displacement[idx] - mean
                    mean += delta / n_rec
                    m2 += delta * (displacement[idx] - mean)
                    self.metrics.update(f'MCMC/chain_{idx}/no_non_diffeomorphic_voxels', int(no_folds[idx]))
                    if no_folds[idx] > 0.001 * no_voxels:  # trainer.py:441-445
                        log(f'chain {idx}, sample {sample_no}: detected {no_folds} voxels where the sampled '
                            f'transformation is not diffeomorphic; exiting..')
                        raise SystemExit(1)
            if self._native is not None and (logged or (self.native_options['period'] is not None and
                                                        is_recorded(sample_no, self.no_iters_burn_in, self.native_options['period']))):
                self.engine.flush()  # as above
                self._log_native(sample_no, output['displacement'], logged and save_samples)
            if self.similarity_options is not None and (logged or (self.similarity_options['period'] is not None and is_recorded(
                    sample_no, self.no_iters_burn_in, self.similarity_options['period']))):
                self.engine.flush()  # as above
                rows = self._image_similarity(fixed, output['im_moving_warped'])
                self._log_similarity([f'MCMC/chain_{idx}/similarity' for idx in range(self.no_chains)], rows)
            if self.local_options is not None and logged:
                local = self._local_maps(fixed, output['im_moving_warped'], ('lncc',))
                lncc = local['lncc']
                self._log_local([f'MCMC/chain_{idx}/local_similarity' for idx in range(self.no_chains)], local['rows'])
            if self.residual_options is not None and logged:
                self.sync_parameters()  # the mixture as it stands at this sample
                self._log_residuals([f'MCMC/chain_{idx}/residuals' for idx in range(self.no_chains)],
                                    self._residual_rows(aux['residuals'], fixed['mask'][:1]))
            due = [r for r in recorders if is_recorded(sample_no, self.no_iters_burn_in, r.period)]
            if due:
                self.engine.flush()  # as above: the buffers hold sample `sample_no` once nothing is pending
            for r in due:
                if r.records == 'seg_warped' and seg_warped is None:
                    seg_warped = self.registration_module(moving['seg'], output['transformation'])
                if r.records == 'lncc' and lncc is None:
                    lncc = self._local_maps(fixed, output['im_moving_warped'], ('lncc',))['lncc']
                if r.records == 'residuals':  # scored under the mixture as it stands at this sample
                    self.sync_parameters()
                    r.state.set_mixture(*residual_check.mixture_terms(data_loss)[2:])
                pick = lambda name: (seg_warped if name == 'seg_warped' else lncc if name == 'lncc' else
                                     aux['residuals'] if name == 'residuals' else
                                     self._dense_velocity(output) if name == 'velocity' else output[name])
                r.state.record(tuple(pick(n) for n in r.records) if isinstance(r.records, tuple) else pick(r.records),
                               **({'step': sample_no} if r.state is self._displacement_modes else {}))
            if self._inverse_consistency is not None:
                ice = self._inverse_consistency
                recorded = any(r.state is ice for r in due)
                if recorded:
                    for space, chains in ice.last_summaries().items():
                        for idx, cs in enumerate(chains):
                            self.metrics.update(f'MCMC/chain_{idx}/ICE/{space}/mean', cs['mean'])
                            self.metrics.update(f'MCMC/chain_{idx}/ICE/{space}/max', cs['max'])
                if logged and (ice_dice or save_samples):
                    # the inverse map of this sample: the recorder's when it just integrated it, else integrated here
                    t_inv, d_inv = ice.last_inverse if recorded else ops.svf_exp_inverse(self._dense_velocity(output), ice.no_steps)
                    if ice_dice:  # the fixed segmentation carried into the moving image's space
                        seg_inv = self.registration_module(fixed['seg'], t_inv)
                        DSC = calc_DSC_GPU(self.no_chains, moving['seg'].expand_as(seg_inv), seg_inv, self.structures_dict)
                        for idx in range(self.no_chains):
                            for j, structure in enumerate(self.structures_dict):
                                self.metrics.update(f'MCMC/chain_{idx}/DSC_inverse/{structure}', float(DSC[idx][j]))
                    if save_samples:
                        for idx in range(self.no_chains):
                            save_field(self.config.save_dirs, spacing, d_inv[idx] * spacing[0],
                                       f'chain_{idx}_sample_{sample_no:07}_displacement_inverse', 'MCMC')
                ice.last_inverse = None  # two fields: not kept between steps
            if self._landmarks is not None and any(r.state is self._landmarks for r in due):
                for name, lp in self._landmarks.directions():
                    for idx, (tre_mean, tre_max) in enumerate(zip(*lp.last_tre())):
                        self.metrics.update(f'MCMC/chain_{idx}/{name}/mean', tre_mean)
                        self.metrics.update(f'MCMC/chain_{idx}/{name}/max', tre_max)
            if checkpoint_period and sample_no % checkpoint_period == 0:
                self._sample_no, self._moments = sample_no, {'mean': mean, 'm2': m2, 'n': n_rec}
                folder = self.config.save_dirs['checkpoints']
                folder.mkdir(parents=True, exist_ok=True)
                self.save_checkpoint(folder / f'checkpoint_{sample_no:07}.pt')
        self.engine.flush()  # a transition dropped by a failed kernel-variant prediction is re-run before anything is saved
        self.displacement_mean = mean
        self.displacement_std = torch.sqrt(m2 / max(n_rec - 1, 1))
        if n_rec > 0 and cfg_trainer.get('save_outputs', True):
            save_displacement_mean_and_std_dev(self.logger, self.config.save_dirs, spacing, self.displacement_mean,
                                               self.displacement_std, moving.get('mask', fixed['mask'])[0].to(mean.dtype), 'MCMC')  # trainer.py:461-462: the MOVING mask
        if self.affine_summary is not None and n_rec > 0 and cfg_trainer.get('save_outputs', True):
            self._save_total_mean(mean, spacing)
        if self._native is not None and n_rec > 0 and cfg_trainer.get('save_outputs', True):
            nat = self._native
            u_mean = transform_coordinates(mean.unsqueeze(0)).contiguous()
            cubic = nat['coeff'] is not None
            out = ops.native_warp(u_mean, nat['grid'], im=None if cubic else nat['moving_im'], fill=nat['fill'],
                                  want_displacement=nat['grid'].mm_scale())
            if cubic:
                out['im'] = bspline.native_warp_cubic(u_mean, nat['grid'], nat['moving_im'], nat['coeff'], nat['fill'])
            save_native_mean(self.logger, self.config.save_dirs, nat['grid'].zooms, out['displacement'][0], out['im'][0, 0], 'MCMC')
        if self.similarity_options is not None and n_rec > 0:
            # the moving image under the posterior-mean displacement: identity + the mean in [-1, 1] coordinates
            ident = init_identity_grid_3D(mean.shape[1:], self.device).permute(0, 4, 1, 2, 3)
            warped = self.registration_module(moving['im'], (ident + transform_coordinates(mean.unsqueeze(0))).contiguous())
            row = self._image_similarity(fixed, warped)[0]
            self._log_similarity(['MCMC/similarity_of_mean'], [row])
            self._similarity_summary('mean', row, f'the mean of {n_rec} samples')
        if self.local_options is not None and n_rec > 0:
            ident = init_identity_grid_3D(mean.shape[1:], self.device).permute(0, 4, 1, 2, 3)
            warped = self.registration_module(moving['im'], (ident + transform_coordinates(mean.unsqueeze(0))).contiguous())
            local = self._local_maps(fixed, warped)
            self._log_local(['MCMC/local_similarity_of_mean'], local['rows'])
            self._local_summary('mean', local['rows'][0], f'the mean of {n_rec} samples')
            if cfg_trainer.get('save_outputs', True) and self.local_options['save']:
                save_local_similarity_of_mean(self.logger, self.config.save_dirs, spacing, local['lncc'][0, 0], local['ssim'][0, 0],
                                              'MCMC')
        for r in recorders:
            r.finish(fixed if r.takes == 'fixed' else masks if r.takes == 'masks' else masks['moving'], spacing,
                     cfg_trainer.get('save_outputs', True))

        # speed test (trainer.py:467-476): 100 x [transition + nearest-neighbour warp of the segmentation]
        n_speed = 100
        torch.cuda.synchronize()
        start = time.perf_counter()
        for _ in range(n_speed):
            _, output, _ = self._SGLD_transition(fixed, moving, data_loss, reg_loss, like_reference=False)
            if 'seg' in moving:
                self.registration_module(moving['seg'], output['transformation'])
        self.engine.flush()
        torch.cuda.synchronize()
        self.MCMC_sampling_speed = self.no_chains * n_speed / (time.perf_counter() - start)
        log(f'\nMCMC sampling speed: {self.MCMC_sampling_speed:.2f} samples/sec')

    def _finish_diagnostics(self, mask, spacing, save_outputs):
        """split-R-hat map and its summary over the moving mask (the std map's mask) -> self.rhat / self.rhat_summary,
        the MCMC/R_hat/* metrics and, with save_outputs, samples/MCMC_rhat[_masked].nii.gz; then, with ESS on, the same for
        the split ESS and MCSE maps"""
        self.rhat, self.rhat_summary = self._chain_moments.rhat(mask)
        s = self.rhat_summary
        for key in ('max', 'mean', 'frac_above_1.01', 'frac_above_1.1'):
            self.metrics.update(f'MCMC/R_hat/{key}', s[key])
        self.logger.info(f'split R-hat over {s["voxels"]} masked voxels ({self.no_chains} chains, '
                         f'{self._chain_moments.n} samples per half): max {s["max"]:.4f}, mean {s["mean"]:.4f}, '
                         f'{100 * s["frac_above_1.01"]:.2f} % above 1.01, {100 * s["frac_above_1.1"]:.2f} % above 1.1')
        if save_outputs:
            save_rhat(self.logger, self.config.save_dirs, spacing, self.rhat, mask, 'MCMC')
        if self.ess_options is None:
            return
        thr = self.ess_options['threshold']
        self.ess, self.mcse, self.ess_summary = self._chain_moments.ess(mask, thr)
        s = self.ess_summary
        for key in ('min', 'mean', f'frac_below_{thr:g}', 'frac_truncated'):
            self.metrics.update(f'MCMC/ESS/{key}', s[key])
        self.logger.info(f'split ESS over {s["voxels"]} masked voxels (max_lag {self._chain_moments.max_lag}): '
                         f'min {s["min"]:.1f}, mean {s["mean"]:.1f}, {100 * s[f"frac_below_{thr:g}"]:.2f} % below {thr:g}, '
                         f'{100 * s["frac_truncated"]:.2f} % truncated')
        if save_outputs:
            save_ess(self.logger, self.config.save_dirs, spacing, self.ess, self.mcse, mask, 'MCMC')

    def _finish_label_posterior(self, fixed, spacing, save_outputs):
        """entropy and MAP maps of the propagated segmentation and their summary -> self.label_entropy / label_map /
        label_summary, the MCMC/seg/* metrics and, with save_outputs, samples/MCMC_seg_*.nii.gz.  The maps live on the fixed
        grid, so the entropy statistics are over the FIXED mask (the std map uses the moving one)."""
        mask = fixed['mask'][0]
        lp = self._label_posterior
        self.label_entropy, self.label_map, self.label_summary = lp.finalize(fixed['seg'][0], mask, spacing)
        s = self.label_summary
        for name, st in s['structures'].items():
            for key in LABEL_STRUCTURE_METRICS:
                self.metrics.update(f'MCMC/seg/{name}/{key}', st[key])
        for key in ('entropy_mean', 'entropy_max', 'ECE'):
            self.metrics.update(f'MCMC/seg/{key}', s[key])
        self.logger.info(f'label posterior of {s["records"]} warped segmentations: entropy over {s["voxels"]} masked voxels '
                         f'mean {s["entropy_mean"]:.4f}, max {s["entropy_max"]:.4f} nats; pooled ECE {s["ECE"]:.4f}')
        if save_outputs:
            prob = lp.probabilities() if self.label_options['prob_maps'] else None
            save_label_posterior(self.logger, self.config.save_dirs, spacing, self.label_entropy, self.label_map, mask, prob,
                                 lp.names, 'MCMC')

    def _finish_surface_posterior(self, fixed, spacing, save_outputs):
        """bias and spread maps of the structures' surfaces and their summary per structure -> self.surface_bias / surface_std /
        surface_summary, the MCMC/surface/* metrics and, with save_outputs and the option's save,
        samples/MCMC_surface_{bias,std}.nii.gz.  The maps live on the fixed grid, so the summary is over the FIXED mask, as for
        the label posterior."""
        sp = self._surface_posterior
        self.surface_bias, self.surface_std, self.surface_summary = sp.finalize(fixed['mask'][0], self.surface_options['coverage'])
        keys = list(SURFACE_METRICS) + [surface_coverage_key(q) for q in self.surface_options['coverage']]
        for name, st in self.surface_summary['structures'].items():
            for key in keys:
                self.metrics.update(f'MCMC/surface/{key}/{name}', st[key])
        seen = [st for st in self.surface_summary['structures'].values() if st['sampled_voxels']]
        self.logger.info(f'surface posterior of {self.surface_summary["records"]} warped segmentations: {len(seen)} structures with a '
                         f'sampled contour' + (f', mean signed distance {np.mean([st["bias"] for st in seen]):.4f}, mean |bias| '
                                               f'{np.mean([st["abs_bias"] for st in seen]):.4f}' if seen else ''))
        if save_outputs and self.surface_options['save']:
            save_surface_posterior(self.logger, self.config.save_dirs, spacing, self.surface_bias, self.surface_std, 'MCMC')

    def _finish_jacobian_posterior(self, fixed, spacing, save_outputs):
        """fold probability, mean and std of log det J and their summary -> self.jacobian_fold_prob / jacobian_logJ_mean /
        jacobian_logJ_std / jacobian_summary, the MCMC/jacobian/* metrics and, with save_outputs, samples/MCMC_fold_prob.nii.gz
        and samples/MCMC_logJ_{mean,std}[_masked].nii.gz.  The maps live on the fixed grid, so the summary is over the FIXED
        mask, as for the label posterior."""
        mask = fixed['mask'][0]
        jp = self._jacobian_posterior
        self.jacobian_fold_prob, self.jacobian_logJ_mean, self.jacobian_logJ_std, self.jacobian_summary = jp.finalize(mask)
        s = self.jacobian_summary
        for key in JACOBIAN_METRICS:
            self.metrics.update(f'MCMC/jacobian/{key}', s[key])
        self.logger.info(f'Jacobian posterior of {s["records"]} transformations over {s["voxels"]} masked voxels: '
                         f'{s["folded_voxels"]} voxels fold in some record ({s["always_folded"]} in all), fold probability '
                         f'max {s["fold_prob_max"]:.4f}, mean {s["fold_prob_mean"]:.3g}; std of log det J mean '
                         f'{s["logJ_std_mean"]:.4f}, max {s["logJ_std_max"]:.4f}')
        if save_outputs:
            save_jacobian_posterior(self.logger, self.config.save_dirs, spacing, self.jacobian_fold_prob, self.jacobian_logJ_mean,
                                    self.jacobian_logJ_std, mask, 'MCMC')

    def _structure_maps(self):
        """the finished per-voxel posterior maps the structure report tabulates: whichever exist -> (names, (M,D,H,W) float32 on
        the device), or ([], None).  The names are the attributes' but for the split R-hat map, 'split_rhat': its maximum would
        collide with the motion key rhat_max"""
        std = self.displacement_std
        cov_std = self.displacement_cov_std
        maps = [('displacement_std_x', None if std is None else std[0]), ('displacement_std_y', None if std is None else std[1]),
                ('displacement_std_z', None if std is None else std[2]),
                ('displacement_std_norm', None if std is None else calc_norm(std.unsqueeze(0))[0, 0]),
                ('split_rhat', self.rhat), ('ess', self.ess), ('mcse', self.mcse), ('label_entropy', self.label_entropy),
                ('jacobian_fold_prob', self.jacobian_fold_prob), ('jacobian_logJ_mean', self.jacobian_logJ_mean),
                ('jacobian_logJ_std', self.jacobian_logJ_std),
                ('displacement_cov_std_major', None if cov_std is None else cov_std[0]),
                ('displacement_cov_anisotropy', self.displacement_cov_anisotropy), ('displacement_ci_width', self.displacement_ci_width),
                ('local_lncc_mean', self.local_lncc_mean), ('residual_nll_mean', self.residual_nll_mean),
                ('comparison_shift', self.comparison_shift), ('comparison_log_std_ratio', self.comparison_log_std_ratio),
                ('comparison_bures', self.comparison_bures), ('comparison_jeffreys', self.comparison_jeffreys)]
        maps = [(name, m) for name, m in maps if m is not None]
        if not maps:
            return [], None
        dims = self._structure_report.dims
        return [name for name, _ in maps], torch.stack([m.to(self.device, torch.float32).reshape(dims) for _, m in maps]).contiguous()

    def _finish_structure_report(self, fixed, spacing, save_outputs):
        """the per-structure table -> self.structure_summary {'records', 'structures': {name: {...}}, 'maps': [names]}: the motion
        keys of structure_report.structure_summary (with coherence / n_eff when trainer.displacement_covariance recorded the same
        steps), then, with the option's "maps", the rows of every finished posterior map; the MCMC/structure/{key}/{structure}
        metrics of the motion keys, one log line per structure and, with save_outputs and the option's save,
        samples/MCMC_structures.csv and samples/MCMC_structure_series.csv.  Runs last: the other recorders have finished"""
        report, opt = self._structure_report, self.structure_options
        cov_trace = None
        if structure_report.with_coherence(self.config['trainer']):
            dc = self._displacement_covariance
            if dc.records != report.records:
                raise RuntimeError(f'structure report: {report.records} records against {dc.records} of the displacement covariance')
            cov_trace = structure_report.covariance_trace(*report.map_stats(dc.comoment[:3].contiguous()), dc.records, report.scale)
        summary, (ints, floats) = report.finalize([float(s) for s in spacing], self.no_chains, cov_trace)
        summary['maps'] = []
        if opt['maps']:
            names, stacked = self._structure_maps()
            if names:
                structure_report.add_map_rows(summary, structure_report.structure_map_rows(*report.map_stats(stacked), names, report.names),
                                              names)
        self.structure_summary = summary
        keys = structure_report.structure_metric_keys(self.config['trainer'])
        for name, row in summary['structures'].items():
            for key in keys:
                self.metrics.update(f'MCMC/structure/{key}/{name}', row[key])
            self.logger.info(f'structure {name}: {row["voxels"]} voxels over {summary["records"]} records; mean shift '
                             f'({row["shift_mean_x"]:.4f}, {row["shift_mean_y"]:.4f}, {row["shift_mean_z"]:.4f}) voxels, its spread '
                             f'major {row["shift_std_major"]:.4f}, total {row["shift_std_total"]:.4f}; |w| mean {row["disp_mean"]:.4f}, '
                             f'max {row["disp_max"]:.4f}; volume ratio {row["vol_ratio_mean"]:.5f} +- {row["vol_ratio_std"]:.5f}, '
                             f'folded {100 * row["fold_frac"]:.3f} %, split R-hat max {row["rhat_max"]:.4f}' +
                             (f'; coherence {row["coherence"]:.4g} (n_eff {row["n_eff"]:.4g})' if 'coherence' in row else ''))
        if save_outputs and opt['save']:
            steps = recorded_steps(self.no_iters_burn_in, self.no_samples_MCMC, opt['period'])
            save_structure_report(self.logger, self.config.save_dirs, structure_report.structures_csv(summary),
                                  structure_report.series_csv(ints, floats, report.names, steps, self.no_chains), 'MCMC')

    # ---------------------------------------------------------------- known-transformation validation
    def _truth_init(self, fixed, moving):
        """trainer.truth -> self._truth, the dense truth (3,D,H,W) on the device in voxels of the registration grid, the unit the
        recorders receive output['displacement'] in.  "simulate": truth.simulate_velocity + truth.known_pair -- the moving triple is
        REPLACED by the fixed one pulled through the inverse of the known transformation; one log line gives the amplitude and the
        truth's own error floor.  "file": truth.read_truth; the moving triple is left alone.  Deterministic: a resumed run makes the
        same truth again.  -> the moving dict the run goes on with"""
        opt = self.truth_options
        dims = tuple(int(n) for n in fixed['im'].shape[2:])
        sp = getattr(self.data_loader, 'im_spacing', None)
        spacing = [1.0, 1.0, 1.0] if sp is None else [float(s) for s in torch.as_tensor(sp).reshape(-1)][:3]
        if opt['source'] == 'simulate':
            v = truth_ops.simulate_velocity(dims, opt['seed'], opt['amplitude'], opt['modes'], opt['max_wavenumber'])
            known, self._truth, info = truth_ops.known_pair(fixed, v, getattr(self.transformation_module, 'no_steps', 12), opt['noise'],
                                                            opt['seed'])
            moving = {**moving, **known}
            self._truth_floor = info
            self.logger.info(f'truth (simulated, seed {opt["seed"]}): velocity amplitude {info["amplitude"]:.4g} voxels, largest '
                             f'displacement component {info["truth_max"]:.4g} voxels; error floor |phi*^-1 o phi* - id| over '
                             f'{info["floor_voxels"]} masked voxels: mean {info["floor_mean"]:.3g}, max {info["floor_max"]:.3g} voxels '
                             f'(an error below it means nothing); the moving image, mask and segmentation are replaced')
        else:
            # the package saves its fields in mm as displacement * spacing[0]: channel c of a file in mm is divided by spacing[c]
            self._truth = torch.as_tensor(truth_ops.read_truth(opt['path'], dims, opt['unit'], spacing)).to(self.device)
            self.logger.info(f'truth (file {opt["path"]}, {opt["unit"]}): largest displacement component '
                             f'{float(self._truth.abs().max()):.4g} voxels')
        if self.config['trainer'].get('save_outputs', True) and opt['save'] and opt['source'] == 'simulate':
            from ..logger import save_field_to_disk
            folder = self.config.save_dirs['samples']
            folder.mkdir(parents=True, exist_ok=True)
            save_field_to_disk(self._truth * spacing[0], str(folder / 'truth_displacement.vtk'), spacing)
        return moving

    def _truth_calibration_init(self, mask):
        """self._truth_calibration over the FIXED mask (the truth lives on the fixed grid), its series sized from the config, and
        the step-0 metrics truth/initial/{rmse,mean,max}: the error of the identity, the update kernel on a zero displacement
        into scratch state.  scale (1, 1, 1): the transition writes the displacement in voxels, and so are the errors"""
        steps = self.no_samples_MCMC // self.truth_options['period']
        self._truth_calibration = TruthCalibration(self._truth, steps * self.no_chains, self.device, mask=mask)
        self._truth_initial = self._truth_calibration.initial_error()
        self.writer.set_step(0)
        for key in truth_ops.INITIAL_METRICS:
            self.metrics.update(f'truth/initial/{key}', self._truth_initial[key])
        self.logger.info('truth: error of the unregistered pair (identity) over the fixed mask: mean '
                         f'{self._truth_initial["mean"]:.4g}, RMS {self._truth_initial["rmse"]:.4g}, max {self._truth_initial["max"]:.4g} voxels')

    def _finish_truth_calibration(self, fixed, spacing, save_outputs):
        """the posterior against the truth over the fixed mask -> self.truth_error / truth_mahalanobis (maps), self.truth_summary
        (truth.calibration_summary), the MCMC/truth/* metrics and, with save_outputs and the option's save,
        samples/MCMC_truth_{error,mahalanobis}[_masked].nii.gz, MCMC_truth_calibration.csv and MCMC_truth_series.csv"""
        tc, opt = self._truth_calibration, self.truth_options
        mask = fixed['mask'][0]
        maps, s, (ints, floats) = tc.finalize(mask, opt['levels'], opt['pit_bins'], opt['rank_bins'], opt['reliability_bins'],
                                              opt['std_floor'], opt['reference'], self._truth_initial, self._truth_floor)
        self.truth_error, self.truth_mahalanobis, self.truth_summary = maps['error'], maps['mahalanobis'], s
        for key in truth_ops.METRIC_KEYS:
            self.metrics.update(f'MCMC/truth/{key}', s[key])
        for key, row in s['coverage'].items():
            self.metrics.update(f'MCMC/truth/coverage_{key}', row['observed'])
        self.logger.info(f'truth calibration of {s["records"]} samples over {s["voxels"]} masked voxels ({s["nonfinite_voxels"]} '
                         f'non-finite, {s["raised_voxels"]} with a raised pivot), reference {s["reference"]}: error of the posterior mean '
                         f'RMS {s["rmse"]:.4g}, mean {s["mean"]:.4g}, max {s["max"]:.4g} voxels (identity: RMS {s["initial_rmse"]:.4g}; '
                         f'error floor of the truth: mean {s["floor_mean"]:.3g}' + (', ABOVE this mean error' if s['below_floor'] else '') +
                         '); coverage ' + ', '.join(f'{row["observed"]:.3f} at {row["nominal"]:g}' for row in s['coverage'].values()) +
                         f'; scale factor {s["scale_factor"]:.4g} (an autocorrelated chain has n_eff < n: part of a factor above 1 is '
                         f'the Monte-Carlo error of the mean); ENCE {s["ence"]:.4g}; PIT chi2 {s["pit_chi2"]:.4g}, KS {s["pit_ks"]:.4g}; '
                         f'z RMS x {s["z_rms_x"]:.3f}, y {s["z_rms_y"]:.3f}, z {s["z_rms_z"]:.3f}')
        if save_outputs and opt['save']:
            steps = recorded_steps(self.no_iters_burn_in, self.no_samples_MCMC, opt['period'])
            save_truth_calibration(self.logger, self.config.save_dirs, spacing, maps, mask, truth_ops.calibration_csv(s),
                                   truth_ops.series_csv(ints, floats, steps, self.no_chains), 'MCMC')

    def _image_init(self, fixed, moving):
        """trainer.image_posterior -> self._image_volumes (S,1,D,H,W) on the device: the moving image as the chain warps it, then
        the extra volumes, read onto the registration grid as the loader reads the moving image and -- with trainer.affine_init
        -- resampled through the same map (affine.resample_pair, as its 'im'); and the floor of the z map, the option's or 1e-3
        of the moving image's intensity range (one host read-back)"""
        opt = self.image_options
        volumes = [moving['im'][:1].to(self.device, torch.float32)]
        for v in opt['volumes']:
            extra = image_posterior.load_volume(v['path'], self.data_loader).to(self.device)
            if self.affine_summary is not None:
                extra = affine.resample_pair({'im': extra}, self.affine_summary['lin'], self.affine_summary['shift'])['im']
            volumes.append(extra)
        self._image_volumes = torch.cat(volumes).contiguous()
        self._image_std_floor = opt['std_floor']
        if self._image_std_floor is None:
            _, (m_lo, m_hi) = ops.intensity_ranges(fixed['im'], moving['im'])
            self._image_std_floor = IMAGE_STD_FLOOR_FRACTION * (m_hi - m_lo)
        self.logger.info(f'image posterior: {len(volumes)} volumes ({", ".join(image_posterior_names(opt))}), '
                         f'{16 * len(volumes)} bytes per voxel; floor of the z map {self._image_std_floor:.6g}')

    def _finish_image_posterior(self, fixed, spacing, save_outputs):
        """mean, std and range maps of every carried volume and, for the moving image with the option's "reference", the z map of
        its posterior mean against the fixed image -> self.image_maps / self.image_summary (keyed by volume name), the
        MCMC/image/{name}/* metrics and, with save_outputs and the option's save,
        samples/MCMC_im_{name}_{mean,std,range}[_masked].nii.gz and samples/MCMC_im_moving_z[_masked].nii.gz.  The maps live on
        the fixed grid, so the summaries are over the FIXED mask, as for the Jacobian posterior."""
        mask = fixed['mask'][0]
        opt = self.image_options
        reference = {'moving': fixed['im'][0, 0]} if opt['reference'] else None
        self.image_maps = self._image_posterior.finalize(mask, reference, self._image_std_floor)
        self.image_summary = {name: volume['summary'] for name, volume in self.image_maps.items()}
        for name, s in self.image_summary.items():
            for key in IMAGE_METRICS + (IMAGE_Z_METRICS if 'z_rms' in s else ()):
                self.metrics.update(f'MCMC/image/{name}/{key}', s[key])
            self.logger.info(f'image posterior of {name!r}: {s["records"]} samples over {s["voxels"]} masked voxels '
                             f'({s["nonfinite_voxels"]} non-finite): mean {s["mean"]:.6g}, std mean {s["std_mean"]:.6g}, max '
                             f'{s["std_max"]:.6g}, widest range {s["range_max"]:.6g}' +
                             (f'; against the fixed image z rms {s["z_rms"]:.4g}, max {s["z_max"]:.4g}, '
                              f'{100 * s["z_gt2"]:.2f} % above 2, {100 * s["z_gt3"]:.2f} % above 3' if 'z_rms' in s else ''))
        if save_outputs and opt['save']:
            save_image_posterior(self.logger, self.config.save_dirs, spacing, self.image_maps, mask, 'MCMC')

    def _finish_displacement_covariance(self, mask, spacing, save_outputs):
        """principal standard deviations (voxels), major direction and fractional anisotropy of the displacement posterior and
        their summary -> self.displacement_cov_std / displacement_cov_direction / displacement_cov_anisotropy /
        displacement_cov_summary, the MCMC/covariance/* metrics and, with save_outputs, samples/MCMC_disp_std_{major,minor}
        [_masked].nii.gz, MCMC_disp_anisotropy[_masked].nii.gz and MCMC_disp_direction.vtk.  The summary is over the mask the
        displacement std map uses."""
        dc = self._displacement_covariance
        (self.displacement_cov_std, self.displacement_cov_direction, self.displacement_cov_anisotropy,
         self.displacement_cov_summary) = dc.finalize(mask)
        s = self.displacement_cov_summary
        for key in COVARIANCE_METRICS:
            self.metrics.update(f'MCMC/covariance/{key}', s[key])
        self.logger.info(f'displacement covariance of {s["records"]} samples over {s["voxels"]} masked voxels '
                         f'({s["nonfinite_voxels"]} non-finite): major std mean {s["std_major_mean"]:.4f}, max '
                         f'{s["std_major_max"]:.4f} voxels, total std mean {s["std_total_mean"]:.4f}; anisotropy mean '
                         f'{s["anisotropy_mean"]:.4f}, max {s["anisotropy_max"]:.4f}; mean |direction| x {s["dir_x"]:.3f}, '
                         f'y {s["dir_y"]:.3f}, z {s["dir_z"]:.3f}')
        if save_outputs:
            save_displacement_covariance(self.logger, self.config.save_dirs, spacing, self.displacement_cov_std,
                                         self.displacement_cov_direction, self.displacement_cov_anisotropy, mask, 'MCMC')

    def _finish_displacement_modes(self, mask, spacing, save_outputs):
        """principal modes of the displacement posterior: eigenvalues, shares, scores and the 1-sigma mode fields ->
        self.displacement_modes_summary / displacement_mode_fields (K,3,D,H,W, normalised coordinates) /
        displacement_mode_scores (n,K), the MCMC/modes/* metrics and, with save_outputs and the option's save,
        samples/MCMC_mode_{k}.vtk, MCMC_modes_explained[_masked].nii.gz, MCMC_modes.csv and MCMC_mode_scores.csv.  The inner
        product of the modes is over the mask the displacement std map uses, fixed when the recorder was created."""
        out = self._displacement_modes.finalize(self.modes_options['modes'])
        s = self.displacement_modes_summary = out['summary']
        self.displacement_mode_fields, self.displacement_mode_scores = out['modes'], out['scores']
        for key in MODES_METRICS:
            self.metrics.update(f'MCMC/modes/{key}', s[key])
        self.logger.info(f'displacement modes of {s["records"]} samples: total variance {s["var_total"]:.6g} voxels^2 over the mask, '
                         f'mode 1 explains {100 * s["explained_1"]:.2f} % (RMS {s["std_1"]:.4f} voxels), the first {s["modes"]} '
                         f'{100 * s["explained_M"]:.2f} %; {s["n90"]} modes reach 90 %, participation ratio '
                         f'{s["participation"]:.2f}; largest split R-hat of the scores {s["rhat_max"]:.4f}')
        if save_outputs and self.modes_options['save']:
            save_displacement_modes(self.logger, self.config.save_dirs, spacing, out, mask, 'MCMC')

    def _finish_displacement_quantiles(self, mask, spacing, save_outputs):
        """quantiles of the displacement posterior (voxels) at the option's probabilities, the width of the band between the
        first and the last and their summary -> self.displacement_quantiles / displacement_ci_width /
        displacement_quantiles_summary, the MCMC/quantiles/* metrics and, with save_outputs, samples/MCMC_disp_q{PP}.vtk and
        MCMC_disp_ci_width[_masked].nii.gz.  The summary is over the mask the displacement std map uses."""
        dq, opt = self._displacement_quantiles, self.quantiles_options
        self.displacement_quantiles, self.displacement_ci_width, self.displacement_quantiles_summary = dq.finalize(opt['probs'], mask)
        s = self.displacement_quantiles_summary
        for key in QUANTILE_METRICS:
            self.metrics.update(f'MCMC/quantiles/{key}', s[key])
        lo, hi = opt['probs'][0], opt['probs'][-1]
        self.logger.info(f'displacement quantiles of {s["records"]} samples over {s["voxels"]} masked voxels: width of the '
                         f'{100 * lo:g} % - {100 * hi:g} % band mean {s["width_mean"]:.4f}, max {s["width_max"]:.4f} voxels '
                         f'(x {s["width_x"]:.4f}, y {s["width_y"]:.4f}, z {s["width_z"]:.4f}); {s["out_of_range_voxels"]} voxels '
                         f'out of range ({100 * s["out_of_range_frac"]:.3f} %), {100 * s["clipped_frac"]:.3f} % of the samples '
                         f'in the open-ended bins')
        if s['out_of_range_frac'] > 0:
            self.logger.warning(f'displacement quantiles: {s["out_of_range_voxels"]} masked voxels have a quantile outside the '
                                f'{opt["bins"]} bins of {opt["bin_width"]:g} voxels around the first sample and are NaN in the '
                                f'maps: raise trainer.displacement_quantiles.bin_width (or bins)')
        if save_outputs:
            save_displacement_quantiles(self.logger, self.config.save_dirs, spacing, opt['probs'], self.displacement_quantiles,
                                        self.displacement_ci_width, mask, 'MCMC')

    def _native_init(self):
        """the pair at its own resolution -> the device, once: the moving image and segmentation that are warped, the fixed
        segmentation they are compared with, the geometry and the value the moving image is padded with"""
        pair = self.data_loader.native()
        to = lambda t: t.unsqueeze(0).contiguous().to(self.device)
        self._native = {'grid': pair['grid'], 'fill': pair['fill']['moving'], 'moving_im': to(pair['moving']['im']),
                        'moving_seg': to(pair['moving']['seg']), 'fixed_seg': to(pair['fixed']['seg']), 'coeff': None}
        g = pair['grid']
        self.logger.info(f'native resolution: {g.shape} voxels of {g.zooms} mm, padded by {g.padding} to {g.padded}, '
                         f'registered at {g.dims}')
        if self.interpolation_options is not None:
            self._native['coeff'] = self._spline_prefilter(self._native['moving_im'], 'the native moving image')
        if self.native_posterior_options is not None:  # what the native posterior is finalized against
            self._native['fixed_im'], self._native['fixed_mask'] = to(pair['fixed']['im']), to(pair['fixed']['mask'])

    def _native_posterior_init(self):
        """trainer.native_posterior -> self._native_posterior over the native pair of _native_init, and the floor of the z map:
        the option's, or 1e-3 of the native moving image's intensity range (one host read-back).  The samples are trilinear
        whatever trainer.output_interpolation says: that option concerns the images that are saved"""
        nat, opt = self._native, self.native_posterior_options
        if opt['labels'] and not self.structures_dict:
            raise ValueError('trainer.native_posterior: "labels" needs structures (the config lists none)')
        np_ = NativePosterior(nat['grid'], self.device, self.structures_dict if opt['labels'] else None,
                              nat['moving_seg'] if opt['labels'] else None, nat['moving_im'] if opt['image'] else None, nat['fill'])
        self._native_posterior = np_
        self._native_std_floor = opt['std_floor']
        if opt['image'] and self._native_std_floor is None:
            lo, hi = nat['moving_im'].aminmax()
            self._native_std_floor = IMAGE_STD_FLOOR_FRACTION * float(hi - lo)
        self.logger.info(f'native posterior: {"labels (" + str(len(np_.labels)) + " structures)" if opt["labels"] else ""}'
                         f'{" and " if opt["labels"] and opt["image"] else ""}{"image" if opt["image"] else ""} on '
                         f'{nat["grid"].shape} voxels, {4 * len(np_.labels) + (16 if opt["image"] else 0)} bytes per native voxel, '
                         f'{np_.state_bytes() / 1e6:.1f} MB on the device')

    def _finish_native_posterior(self, fixed, spacing, save_outputs):
        """entropy and MAP maps of the propagated native segmentation, mean / std / range / z maps of the native moving image and
        their summaries over the NATIVE fixed mask -> self.native_posterior_maps / native_posterior_summary, the MCMC/native/seg/*
        and MCMC/native/image/moving/* metrics (the volumes in mm^3 under the header zooms) and, with save_outputs,
        samples/MCMC_seg_{entropy,MAP}_native.nii.gz[, MCMC_seg_prob_{structure}_native.nii.gz] and
        samples/MCMC_im_moving_{mean,std,range,z}_native.nii.gz with the header zooms.  `fixed` and `spacing` belong to the
        registration grid and are not used"""
        nat, opt, np_ = self._native, self.native_posterior_options, self._native_posterior
        self.native_posterior_maps = np_.finalize(nat['fixed_seg'][0, 0] if opt['labels'] else None, nat['fixed_im'][0, 0],
                                                  nat['fixed_mask'][0, 0], self._native_std_floor or 0.0)
        self.native_posterior_summary = {part: maps['summary'] for part, maps in self.native_posterior_maps.items()}
        if opt['labels']:
            s = self.native_posterior_summary['labels']
            for name, st in s['structures'].items():
                for key in LABEL_STRUCTURE_METRICS:
                    self.metrics.update(f'MCMC/native/seg/{key}/{name}', st[key])
            for key in ('entropy_mean', 'entropy_max', 'ECE'):
                self.metrics.update(f'MCMC/native/seg/{key}', s[key])
            self.logger.info(f'native label posterior of {s["records"]} warped segmentations: entropy over {s["voxels"]} masked '
                             f'voxels mean {s["entropy_mean"]:.4f}, max {s["entropy_max"]:.4f} nats; pooled ECE {s["ECE"]:.4f}')
        if opt['image']:
            s = self.native_posterior_summary['image']
            for key in NATIVE_POSTERIOR_IMAGE_METRICS:
                self.metrics.update(f'MCMC/native/image/moving/{key}', s[key])
            self.logger.info(f'native image posterior: {s["records"]} samples over {s["voxels"]} masked voxels '
                             f'({s["nonfinite_voxels"]} non-finite): std mean {s["std_mean"]:.6g}, max {s["std_max"]:.6g}; against '
                             f'the fixed image z rms {s["z_rms"]:.4g}, {100 * s["z_gt2"]:.2f} % above 2')
        if save_outputs:
            prob = np_.probabilities() if opt['labels'] and opt['prob_maps'] else None
            save_native_posterior(self.logger, self.config.save_dirs, nat['grid'].zooms, self.native_posterior_maps, prob, np_.names,
                                  'MCMC')

    def _log_native(self, sample_no, displacement, save):
        """the sample carried to the image's own voxel grid in ONE launch: the warped native moving segmentation -> the metrics
        MCMC/chain_i/native/{DSC,ASD[,HD,HD{q}]}/{structure}, the surface distances in mm under the header zooms; with `save`
        also what trainer.native_resolution.save lists.  displacement: (C,3,*dims) in voxels of the registration grid, as the
        transition returns it"""
        nat, opt = self._native, self.native_options
        grid = nat['grid']
        want = set(opt['save']) if save else set()
        cubic = nat['coeff'] is not None and 'im' in want  # the saved image alone: the labels stay nearest-neighbour
        u = transform_coordinates(displacement).contiguous()
        out = ops.native_warp(u, grid, seg=nat['moving_seg'], im=nat['moving_im'] if 'im' in want and not cubic else None,
                              fill=nat['fill'], want_displacement=grid.mm_scale() if 'displacement' in want else None)
        if cubic:
            out['im'] = bspline.native_warp_cubic(u, grid, nat['moving_im'], nat['coeff'], nat['fill'])
        if self.structures_dict:
            self._log_segmentation_metrics([f'MCMC/chain_{idx}/native' for idx in range(self.no_chains)], nat['fixed_seg'],
                                           out['seg'], grid.spacing_xyz())
        for idx in range(self.no_chains if save else 0):
            save_native_sample(self.config.save_dirs, grid.zooms, sample_no, idx, im=out['im'][idx, 0] if 'im' in want else None,
                               seg=out['seg'][idx, 0] if 'seg' in want else None,
                               displacement_mm=out['displacement'][idx] if 'displacement' in want else None)

    def _similarity_init(self, fixed, moving):
        """the two intensity ranges the histograms are binned over: the finite min / max of the fixed and of the moving image
        (trilinear interpolation with border padding cannot leave the moving range); one host read-back"""
        self._similarity_ranges = ops.intensity_ranges(fixed['im'], moving['im'])
        (f_lo, f_hi), (m_lo, m_hi) = self._similarity_ranges
        self.logger.info(f'image similarity: {self.similarity_options["bins"]} bins over [{f_lo:g}, {f_hi:g}] (fixed) and '
                         f'[{m_lo:g}, {m_hi:g}] (moving)')

    def _image_similarity(self, fixed, moving_im):
        """-> one dict per volume of moving_im (utils.calc_image_similarity) against fixed['im'] under fixed['mask'], all chains
        in one call; one warning per run when a call clipped an intensity or met a non-finite one"""
        rows = calc_image_similarity(fixed['im'], moving_im.contiguous(), fixed['mask'][:1], self.similarity_options['bins'],
                                     *self._similarity_ranges)
        if not self._similarity_warned and any(r['n_clipped'] > 0 or r['n_nonfinite'] > 0 for r in rows):
            self._similarity_warned = True
            self.logger.warning(f'image similarity: {max(r["n_clipped"] for r in rows)} voxels outside the intensity ranges (counted '
                                f'in the end bins) and {max(r["n_nonfinite"] for r in rows)} with a non-finite intensity (left out); '
                                f'not reported again in this run')
        return rows

    def _log_similarity(self, prefixes, rows):
        for prefix, row in zip(prefixes, rows):
            for key in SIMILARITY_METRICS:
                self.metrics.update(f'{prefix}/{key}', row[key.lower()])

    def _similarity_summary(self, name, row, what):
        """self.similarity_summary[name] = the four numbers and the voxel count, and one log line"""
        if self.similarity_summary is None:
            self.similarity_summary = {}
        self.similarity_summary[name] = {'n': row['n'], **{key: row[key.lower()] for key in SIMILARITY_METRICS}}
        self.logger.info(f'image similarity of {what} over {row["n"]} masked voxels: ' +
                         ', '.join(f'{key} {row[key.lower()]:.6g}' for key in SIMILARITY_METRICS))

    def _log_similarity_unregistered(self, fixed, moving):
        """step 0: the unregistered pair under VI/train/similarity/*, with or without segmentations"""
        self._similarity_init(fixed, moving)
        self.writer.set_step(0)
        row = self._image_similarity(fixed, moving['im'][:1])[0]
        self._log_similarity(['VI/train/similarity'], [row])
        self._similarity_summary('unregistered', row, 'the unregistered pair')

    def _local_init(self, fixed, moving):
        """the two intensity ranges that give the flatness floors and the SSIM constants: the finite min / max of the fixed and
        of the moving image (trilinear interpolation with border padding cannot leave the moving range); one host read-back"""
        if self._local_ranges is not None:
            return
        self._local_ranges = ops.intensity_ranges(fixed['im'], moving['im'])
        floor_f, floor_m, c1, c2 = ops.local_similarity_constants(*self._local_ranges)
        r = self.local_options['radius']
        self.logger.info(f'local similarity: windows of {2 * r + 1}^3 voxels, a window is flat below a variance of {floor_f:.3g} '
                         f'(fixed) / {floor_m:.3g} (moving); SSIM constants {c1:.3g}, {c2:.3g}')

    def _local_maps(self, fixed, moving_im, want=('lncc', 'ssim')):
        """ops.local_similarity of every volume of moving_im against fixed['im'] under fixed['mask'], all chains in one call ->
        its dict plus 'rows': one dict of statistics per volume (utils.local_similarity_rows); one warning per run when a
        window held a non-finite value"""
        out = ops.local_similarity(fixed['im'], moving_im.contiguous(), fixed['mask'][:1], self.local_options['radius'],
                                   *self._local_ranges, want=want)
        out['rows'] = local_similarity_rows(out['stats'])
        if not self._local_warned and any(r['n_nonfinite'] > 0 for r in out['rows']):
            self._local_warned = True
            self.logger.warning(f'local similarity: {max(r["n_nonfinite"] for r in out["rows"])} masked voxels whose window holds a '
                                f'non-finite intensity (NaN in the maps, left out of the statistics); not reported again in this run')
        return out

    def _log_local(self, prefixes, rows):
        for prefix, row in zip(prefixes, rows):
            for key, column in LOCAL_METRICS:
                self.metrics.update(f'{prefix}/{key}', row[column])

    def _local_summary(self, name, row, what):
        """self.local_similarity_summary[name] = the statistics of one pair of maps, and one log line"""
        if self.local_similarity_summary is None:
            self.local_similarity_summary = {}
        self.local_similarity_summary[name] = dict(row)
        self.logger.info(f'local similarity of {what} over {row["n"]} masked voxels ({row["n_flat"]} flat): LNCC mean '
                         f'{row["lncc_mean"]:.6g}, min {row["lncc_min"]:.6g}; SSIM mean {row["ssim_mean"]:.6g}, min '
                         f'{row["ssim_min"]:.6g}')

    def _log_local_unregistered(self, fixed, moving):
        """step 0: the unregistered pair under VI/train/local_similarity/*, with or without segmentations"""
        self._local_init(fixed, moving)
        self.writer.set_step(0)
        row = self._local_maps(fixed, moving['im'][:1], ())['rows'][0]
        self._log_local(['VI/train/local_similarity'], [row])
        self._local_summary('unregistered', row, 'the unregistered pair')

    def _finish_local_similarity(self, fixed, spacing, save_outputs):
        """mean and minimum of the recorded LNCC maps and their summary -> self.local_lncc_mean / local_lncc_min /
        local_similarity_summary['posterior'] and, with save_outputs and the option's save,
        samples/MCMC_lncc_{mean,min}[_masked].nii.gz.  The maps live on the fixed grid: the summary is over the FIXED mask."""
        mask = fixed['mask'][0]
        self.local_lncc_mean, self.local_lncc_min, s = self._local_similarity.finalize(mask)
        if self.local_similarity_summary is None:
            self.local_similarity_summary = {}
        self.local_similarity_summary['posterior'] = s
        self.logger.info(f'LNCC posterior of {s["records"]} samples over {s["voxels"]} masked voxels ({s["empty_voxels"]} never '
                         f'defined): mean of the mean map {s["lncc_mean"]:.6g}, its minimum {s["lncc_mean_min"]:.6g}; lowest sample '
                         f'{s["lncc_min"]:.6g}')
        if save_outputs and self.local_options['save']:
            save_local_similarity_posterior(self.logger, self.config.save_dirs, spacing, self.local_lncc_mean, self.local_lncc_min,
                                            mask, 'MCMC')

    def _residual_init(self, fixed, moving):
        """the half range of the residual histograms, taken once and kept: the option's, else the largest finite |z| of the
        unregistered pair's residual under the fixed mask (one host read-back)"""
        if self._residual_range is not None:
            return
        h = self.residual_options['range']
        if h is None:
            z = self.losses['data']['loss'].map(fixed['im'][:1], moving['im'][:1]).contiguous()
            h = float(residual_check.residual_histogram(z, fixed['mask'][:1], 1.0, 2)['sums'][0, 3])
            if not (math.isfinite(h) and h > 0):
                self.logger.warning(f'residual check: the unregistered pair has no non-zero finite residual under the mask '
                                    f'(max |z| = {h}); binning over [-1, 1]')
                h = 1.0
        self._residual_range = float(torch.tensor(h, dtype=torch.float32))
        self.logger.info(f'residual check: {self.residual_options["bins"]} bins over [-{self._residual_range:g}, '
                         f'{self._residual_range:g}]')

    def _residual_rows(self, residuals, mask):
        """utils.calc_residual_check of (C,1,D,H,W) residuals under `mask` against the data loss as it stands -> one dict per
        chain; one warning per run when a residual was clipped or not finite"""
        rows = calc_residual_check(residuals, mask, self.losses['data']['loss'], self._residual_range, self.residual_options['bins'])
        if not self._residual_warned and any(r['n_clipped'] > 0 or r['n_nonfinite'] > 0 for r in rows):
            self._residual_warned = True
            self.logger.warning(f'residual check: {max(r["n_clipped"] for r in rows)} residuals beyond +-{self._residual_range:g} '
                                f'(counted in the end bins) and {max(r["n_nonfinite"] for r in rows)} non-finite ones (left out); '
                                f'not reported again in this run')
        return rows

    def _log_residuals(self, prefixes, rows):
        for prefix, row in zip(prefixes, rows):
            for key, value in residual_metrics(row).items():
                self.metrics.update(f'{prefix}/{key}', value)

    def _residual_summary(self, name, row, what):
        """self.residual_summary[name] = one fit, and one log line"""
        if self.residual_summary is None:
            self.residual_summary = {}
        self.residual_summary[name] = row
        fit = row.get('fit', row)
        self.logger.info(f'residuals of {what} against the mixture over {fit["n"]} values: KL {fit["kl"]:.4g}, TV {fit["tv"]:.4g}, '
                         f'KS {fit["ks"]:.4g}; std {fit["std"]:.4g} (model {fit["std_model"]:.4g}), kurtosis {fit["kurtosis"]:.4g} '
                         f'(model {fit["kurtosis_model"]:.4g}), beyond the range {fit["tail"]:.3g} (model {fit["tail_model"]:.3g})')

    def _log_residuals_unregistered(self, fixed, moving):
        """step 0: the unregistered pair's residual against the mixture as the GMM initialisation left it, under
        VI/train/residuals/*"""
        self._residual_init(fixed, moving)
        self.writer.set_step(0)
        z = self.losses['data']['loss'].map(fixed['im'][:1], moving['im'][:1])
        row = self._residual_rows(z, fixed['mask'][:1])[0]
        self._log_residuals(['VI/train/residuals'], [row])
        self._residual_summary('unregistered', row, 'the unregistered pair')

    def _finish_residual_check(self, fixed, spacing, save_outputs):
        """the recorded histogram pooled over chains and records against the final mixture, and the NLL map over the FIXED mask
        -> self.residual_nll_mean, residual_summary['posterior'], the MCMC/residuals/* metrics and, with save_outputs and the
        option's save, samples/MCMC_residual_hist.csv and samples/MCMC_nll_mean[_masked].nii.gz"""
        rc, mask = self._residual_check, fixed['mask'][0]
        self.sync_parameters()
        std, proportions, _, _ = residual_check.mixture_terms(self.losses['data']['loss'])
        self.residual_nll_mean, s = rc.finalize(std, proportions, mask)
        self._log_residuals(['MCMC/residuals'], [s['fit']])
        if rc.nll_map:
            self.metrics.update('MCMC/residuals/nll_mean', s['nll']['nll_mean'])
            self.metrics.update('MCMC/residuals/nll_max', s['nll']['nll_max'])
            self.logger.info(f'NLL map of {s["records"]} samples over {s["nll"]["voxels"]} masked voxels ({s["nll"]["empty_voxels"]} '
                             f'without a finite residual): mean {s["nll"]["nll_mean"]:.6g}, max {s["nll"]["nll_max"]:.6g}')
        self._residual_summary('posterior', s, f'{s["records"]} recorded volumes')
        if save_outputs and self.residual_options['save']:
            p, _ = residual_check.model_probabilities(rc.half_range, rc.bins, std, proportions)
            save_residual_histogram(self.logger, self.config.save_dirs, residual_check.bin_edges(rc.half_range, rc.bins), rc.hist, p,
                                    'MCMC')
            if rc.nll_map:
                save_residual_nll(self.logger, self.config.save_dirs, spacing, self.residual_nll_mean, mask, 'MCMC')

    def _comparison_init(self, dims):
        """trainer.posterior_comparison -> self._posterior_comparison, once: the VI test stage makes it, or -- on a resume
        without a VI stage -- the MCMC stage, whose checkpoint then brings the VI side"""
        if self._posterior_comparison is None:
            self._posterior_comparison = PosteriorComparison(dims, self.device)
        return self._posterior_comparison

    def _finish_posterior_comparison(self, mask, spacing, save_outputs):
        """the VI posterior (A) against the pooled MCMC samples (B): mean shift, log ratio of the total spreads, Bures distance
        and Jeffreys divergence of the two per-voxel Gaussians, in voxels, and their summary -> self.comparison_shift /
        comparison_log_std_ratio / comparison_bures / comparison_jeffreys / comparison_summary, the MCMC/vs_VI/* metrics and,
        with save_outputs, samples/MCMC_vs_VI_{shift,log_std_ratio,bures,jeffreys}[_masked].nii.gz.  The summary is over the
        mask the displacement std map uses."""
        pc = self._posterior_comparison
        maps, s = pc.finalize(mask, std_floor=self.comparison_options['std_floor'])
        self.comparison_shift, self.comparison_log_std_ratio = maps['shift'], maps['log_std_ratio']
        self.comparison_bures, self.comparison_jeffreys = maps['bures'], maps['jeffreys']
        self.comparison_summary = s
        for key in COMPARISON_METRICS:
            self.metrics.update(f'MCMC/vs_VI/{key}', s[key])
        self.logger.info(f'VI ({s["records_vi"]} samples) against MCMC ({s["records_mcmc"]} samples) over {s["voxels"]} masked voxels '
                         f'({s["nonfinite_voxels"]} non-finite, {s["floored_voxels"]} with a floored eigenvalue): mean shift '
                         f'{s["shift_mean"]:.4f}, max {s["shift_max"]:.4f} voxels; total std VI {s["std_total_vi"]:.4f}, MCMC '
                         f'{s["std_total_mcmc"]:.4f}, ratio {s["std_ratio"]:.4f} (VI the narrower at '
                         f'{100 * s["frac_vi_narrower"]:.2f} % of the voxels); Bures mean {s["bures_mean"]:.4f}, 2-Wasserstein mean '
                         f'{s["w2_mean"]:.4f}, max {s["w2_max"]:.4f} voxels; Jeffreys mean {s["jeffreys_mean"]:.4g}, max '
                         f'{s["jeffreys_max"]:.4g}')
        if save_outputs:
            save_posterior_comparison(self.logger, self.config.save_dirs, spacing, maps, mask, 'MCMC')

    def _landmarks_init(self, dims):
        """trainer.landmarks -> self._landmarks (diagnostics.LandmarkPair), once: the landmark files' voxel indices carried to
        [-1,1] coordinates of the registration grid -- through the native geometry when the loader has native volumes (the TRE
        is then in mm under the header zooms), else as indices of the registration grid (the TRE is in its voxels)"""
        from ..data_loader.synthetic import synthetic_landmarks
        from ..landmarks import grid_points, registration_grid_points
        if self._landmarks is not None:
            return
        opt, dims = self.landmark_options, tuple(int(d) for d in dims)
        native = getattr(self.data_loader, 'native', None)
        if native is not None:
            grid = self._native['grid'] if self._native is not None else native()['grid']
            fixed_pts, moving_pts = grid_points(opt['fixed'], grid), grid_points(opt['moving'], grid)
            scale, self._landmark_unit = grid.mm_scale(), 'mm'
        else:
            fixed_idx, moving_idx = synthetic_landmarks(dims) if opt['synthetic'] else (opt['fixed'], opt['moving'])
            fixed_pts, moving_pts = registration_grid_points(fixed_idx, dims), registration_grid_points(moving_idx, dims)
            scale, self._landmark_unit = voxel_scale(dims), 'voxels'
        new = lambda points, targets: LandmarkPosterior(points, targets, dims, self.device, scale=scale)
        self._landmarks = LandmarkPair(new(fixed_pts, moving_pts), new(moving_pts, fixed_pts) if opt['inverse'] else None,
                                       getattr(self.transformation_module, 'no_steps', 12))
        self.logger.info(f'landmarks: {len(fixed_pts)} pairs, TRE in {self._landmark_unit}' +
                         (', both directions' if opt['inverse'] else ''))

    def _log_landmarks_unregistered(self, fixed):
        """step 0: the TRE of the unregistered pair (zero displacement) under VI/train/TRE/{mean,median,max}"""
        self._landmarks_init(fixed['im'].shape[2:])
        e = self._landmarks.forward.initial_tre().numpy()
        self.writer.set_step(0)
        for key, value in (('mean', e.mean()), ('median', np.median(e)), ('max', e.max())):
            self.metrics.update(f'VI/train/TRE/{key}', float(value))
        self.logger.info(f'TRE of the unregistered pair over {e.size} landmarks: mean {e.mean():.4g}, median {np.median(e):.4g}, '
                         f'max {e.max():.4g} {self._landmark_unit}')

    def _finish_landmarks(self, masks, spacing, save_outputs):
        """the per-landmark table and the summary of the landmark posterior -> self.landmark_summary ({'unit', 'TRE': {...,
        'columns', 'table'}[, 'TRE_inverse': {...}]}), the MCMC/TRE[_inverse]/* metrics and, with save_outputs,
        samples/MCMC_landmarks[_inverse].csv and samples/MCMC_landmarks[_inverse]_mean.vtk.  The masks are not used: a landmark is a
        point, not a voxel."""
        levels = self.landmark_options['coverage_levels']
        self.landmark_summary = {'unit': self._landmark_unit}
        for name, lp in self._landmarks.directions():
            table, s = lp.finalize(levels)
            for key in LANDMARK_METRICS:
                self.metrics.update(f'MCMC/{name}/{key}', s[key])
            for level, value in s['coverage'].items():
                self.metrics.update(f'MCMC/{name}/coverage_{level}', value)
            self.metrics.update(f'MCMC/{name}/error_spread_correlation', s['error_spread_correlation'])
            self.landmark_summary[name] = {**s, 'columns': list(ops.LANDMARK_COLUMNS), 'table': table.tolist()}
            self.logger.info(f'landmark posterior ({name}) of {s["records"]} samples at {s["landmarks"]} landmarks '
                             f'({s["empty_landmarks"]} without a finite sample), in {self._landmark_unit}: TRE of the mean '
                             f'{s["of_mean_mean"]:.4g} (median {s["of_mean_median"]:.4g}, max {s["of_mean_max"]:.4g}), of the samples '
                             f'{s["sample_mean"]:.4g} (max {s["sample_max"]:.4g}); coverage ' +
                             ', '.join(f'{v:.3f} at {k}' for k, v in s['coverage'].items()) +
                             f'; error / spread correlation {s["error_spread_correlation"]:.3f}')
            if save_outputs:
                save_landmarks(self.logger, self.config.save_dirs, lp.mean_points().cpu().numpy(), table, ops.LANDMARK_COLUMNS,
                               self._landmark_unit, 'MCMC', '' if name == 'TRE' else '_inverse')

    def _dense_velocity(self, output):
        """the velocity field the forward exponential of this transition integrated, (C,3,D,H,W) in voxel units: the recorded
        sample itself for SVF_3D, its B-spline up-sampling for SVFFD_3D"""
        v = output['curr_state']
        if self.config['transformation_module']['type'] == 'SVFFD_3D':
            return ops.ffd_up(v.contiguous(), tuple(self._outputs['displacement'].shape[2:]),
                              tuple(self.config['transformation_module']['args']['cps']))
        return v

    def _finish_inverse_consistency(self, masks, spacing, save_outputs):
        """mean and peak maps of the inverse-consistency error (voxels) in both orders and their summaries -> self.ice_summary
        ({'records', 'fixed': {...}, 'moving': {...}}), the MCMC/ICE/{fixed,moving}/* metrics and, with save_outputs,
        samples/MCMC_ICE_{fixed,moving}_{mean,max}[_masked].nii.gz.  |phi^-1 o phi - id| lives on the fixed grid and is summarised
        over the FIXED mask; |phi o phi^-1 - id| lives on the moving grid and is summarised over the MOVING mask."""
        ice, thr = self._inverse_consistency, self.ice_options['threshold']
        summary = ice.finalize(masks, thr)
        self.ice_summary = {'records': ice.records, 'threshold': thr, **summary}
        for space in ICE_SPACES:
            s = summary[space]
            for key in ('mean', 'max', f'frac_above_{thr:g}'):
                self.metrics.update(f'MCMC/ICE/{space}/{key}', s[key])
            self.logger.info(f'inverse consistency of {s["records"]} samples on the {space} grid over {s["voxels"]} masked voxels '
                             f'({s["nonfinite_voxels"]} non-finite): mean {s["mean"]:.3g}, max {s["max"]:.3g} voxels, '
                             f'{100 * s[f"frac_above_{thr:g}"]:.3f} % of the voxels above {thr:g} in some sample')
        if save_outputs:
            save_inverse_consistency(self.logger, self.config.save_dirs, spacing, ice.mean, ice.peak, masks, 'MCMC')

    def _run_model(self):
        for fixed, moving, var_params_q_v in self.data_loader:
            fixed = {k: v.to(self.device) for k, v in fixed.items()}
            moving = {k: v.to(self.device) for k, v in moving.items()}
            if self.truth_options is not None:
                moving = self._truth_init(fixed, moving)
            if self.auto_mask_options is not None:
                self._auto_mask(fixed, moving)
            if self.affine_options is not None:
                moving = self._affine_init(fixed, moving)
            if self.image_options is not None:
                self._image_init(fixed, moving)
            self._engine_init(fixed, moving)
            self._GMM_init(fixed, moving, var_params_q_v)
            self._metrics_init(fixed, moving)
            var_params_q_v = {k: v.to(self.device) for k, v in var_params_q_v.items()}
            self._sobolev_init()
            self._init_optimizers()
            if self.VI:
                start = time.perf_counter()
                self._run_VI(fixed, moving, var_params_q_v)
                torch.cuda.synchronize()
                self.logger.info(f'VI took {time.perf_counter() - start:.2f} seconds')
                self._test_VI(fixed, moving, var_params_q_v)
                self._push_hyperparameters_to_engine()
                var_params_q_v = {k: v.detach() for k, v in var_params_q_v.items()}
            if self.MCMC:
                self._run_MCMC(fixed, moving, var_params_q_v)
