"""Jacobian posterior, host side: the hand-checked case of the definitions against the numpy restatement, the rounding bound
and the tolerances the device is held to (checked here with float32 numpy on the GPU test's own inputs), the config option
and its refusals, the metric names, and the parts of the surface that need no device."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.diagnostics import JACOBIAN_METRICS, JacobianPosterior, jacobian_posterior_options, jacobian_summary
from tests._jacobian_posterior import (CASES, DELTA, RECIPES, case_seed, det_np, draw_records, fold_bounds, identity_np,
                                       jacobian_posterior_np, maps_np, summary_np, tolerances, welford_f32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {'no_samples_MCMC': 80, 'log_period_MCMC': 10, 'no_chains': 2}
LN2 = math.log(2.0)


def hand_checked_records(shape=(3, 4, 5)):
    """the identity (det 1), x stretched by 2 (det 2), x mirrored (det -1, folded), uniform scale 1/2 (det 1/8)"""
    ident = identity_np(shape)
    scale = lambda sx, sy, sz: ident * np.array([sx, sy, sz], dtype=np.float32).reshape(3, 1, 1, 1)
    return np.stack([ident, scale(2, 1, 1), scale(-1, 1, 1), scale(0.5, 0.5, 0.5)])


HAND_MEAN = -2 * LN2 / 3
HAND_STD = math.sqrt(((0 - HAND_MEAN) ** 2 + (LN2 - HAND_MEAN) ** 2 + (-3 * LN2 - HAND_MEAN) ** 2) / 2)


def _config(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['trainer'].update(trainer_over)
    return ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')


# ---------------------------------------------------------------- the restatement
def test_hand_checked_case_of_the_restatement():
    ref = jacobian_posterior_np(hand_checked_records())
    for r, want in enumerate((1.0, 2.0, -1.0, 0.125)):
        assert np.abs(ref['det'][r] - want).max() <= 1e-6  # linspace in float32: the grid is not exactly uniform
    assert (ref['folds'] == 1).all() and (ref['k'] == 3).all()
    assert np.array_equal(ref['fold_prob'], np.full((3, 4, 5), 0.25))
    assert np.abs(ref['logJ_mean'] - HAND_MEAN).max() <= 1e-6
    assert np.abs(ref['logJ_std'] - HAND_STD).max() <= 1e-6
    s = ref['summary']
    assert (s['voxels'], s['folded_voxels'], s['always_folded'], s['fold_records']) == (60, 60, 0, 60)
    assert s['fold_prob_max'] == 0.25 and s['fold_prob_mean'] == 0.25
    assert s['logJ_mean_min'] == pytest.approx(HAND_MEAN, abs=1e-6) and s['logJ_mean_max'] == pytest.approx(HAND_MEAN, abs=1e-6)
    assert s['logJ_std_mean'] == pytest.approx(HAND_STD, abs=1e-6) and s['logJ_std_max'] == pytest.approx(HAND_STD, abs=1e-6)


def test_folded_rule_nan_zero_and_empty_cases():
    ident = identity_np((2, 3, 4))
    flat = ident.copy()
    flat[0] = 0.0  # x collapsed: det == 0 exactly, folded although its log is -inf and not NaN
    bad = ident.copy()
    bad[1, 1, 1, 1] = np.nan
    ref = jacobian_posterior_np(np.stack([flat, bad]))
    assert (ref['det'][0] == 0).all() and (ref['folded'][0]).all()
    assert np.isnan(ref['det'][1]).any() and np.array_equal(ref['folded'][1], np.isnan(ref['det'][1]))
    # every record folded: NaN maps, always_folded counts it; an empty mask gives NaN
    ref = jacobian_posterior_np(np.stack([flat, flat]), mask=np.zeros((2, 3, 4), dtype=bool))
    assert (ref['fold_prob'] == 1).all() and np.isnan(ref['logJ_mean']).all() and np.isnan(ref['logJ_std']).all()
    assert ref['summary']['voxels'] == 0 and all(math.isnan(ref['summary'][k]) for k in
                                                 ('fold_prob_max', 'fold_prob_mean', 'logJ_mean_min', 'logJ_std_mean'))
    s = summary_np(ref['folds'], 2, ref['fold_prob'], ref['logJ_mean'], ref['logJ_std'])
    assert s['always_folded'] == 24 and s['fold_prob_max'] == 1.0 and math.isnan(s['logJ_std_max'])
    # one valid record: std 0 (the displacement std's denominator convention, max(k - 1, 1))
    ref = jacobian_posterior_np(np.stack([flat, ident]))
    assert (ref['logJ_std'] == 0).all() and (ref['fold_prob'] == 0.5).all()


@pytest.mark.parametrize('recipe', RECIPES)
@pytest.mark.parametrize('C,steps,shape', CASES)
def test_the_bound_is_real_on_the_inputs_of_the_gpu_test(C, steps, shape, recipe):
    """a float32 evaluation of det in the kernel's operation order stays within e; outside the band |det| < DELTA it never
    disagrees in sign; the band holds at most 0.5 % of the voxel-records; and the kernel's float32 recurrences stay within the
    tolerances the device is held to"""
    n = C * steps
    rec = draw_records(recipe, n, shape, case_seed(C, steps, shape, recipe))
    ref = jacobian_posterior_np(rec)
    det32, _ = det_np(rec, np.float32)
    assert det32.dtype == np.float32
    err = np.abs(det32.astype(np.float64) - ref['det'])
    assert (err <= ref['e']).all(), float((err / ref['e']).max())
    band = np.abs(ref['det']) < DELTA
    assert band.mean() <= 0.005
    assert not (((det32 > 0) != (ref['det'] > 0)) & ~band).any()
    folds, mean, m2 = welford_f32(det32)
    lo, hi = fold_bounds(ref['det'])
    assert ((lo <= folds) & (folds <= hi)).all()
    clear, tol_mean, tol_root, tol_std = tolerances(ref)
    v = clear & (ref['k'] > 0)
    assert np.array_equal(folds[clear], ref['folds'][clear])
    assert (np.abs(mean.astype(np.float64) - ref['mean'])[v] <= tol_mean[v]).all()
    assert (np.abs(np.sqrt(m2.astype(np.float64)) - np.sqrt(ref['m2']))[v] <= tol_root[v]).all()
    _, _, std = maps_np(folds, mean, m2, n)
    assert (np.abs(std - ref['logJ_std'])[v] <= tol_std[v]).all()
    if recipe == 'folding' and min(shape) >= 5:
        assert 0.09 <= ref['folded'].mean() <= 0.44


# ---------------------------------------------------------------- the config option
def test_option_values():
    assert jacobian_posterior_options(BASE) is None
    for off in (False, None):
        assert jacobian_posterior_options({**BASE, 'jacobian_posterior': off}) is None
    assert jacobian_posterior_options({**BASE, 'jacobian_posterior': True}) == {'period': 10}
    assert jacobian_posterior_options({**BASE, 'jacobian_posterior': {}}) == {'period': 10}
    assert jacobian_posterior_options({**BASE, 'jacobian_posterior': {'period': 3}}) == {'period': 3}
    assert jacobian_posterior_options({**BASE, 'jacobian_posterior': {'period': 80}}) == {'period': 80}


@pytest.mark.parametrize('opt', [{'period': 0}, {'period': -2}, {'period': 2.5}, {'period': 2.0}, {'period': '2'},
                                 {'period': True}, {'period': None}, {'periods': 2}, {'period': 2, 'maps': True},
                                 {'prob_maps': True}, 'yes', 1, [2]])
def test_option_refusals(opt):
    with pytest.raises(ValueError, match='jacobian_posterior'):
        jacobian_posterior_options({**BASE, 'jacobian_posterior': opt})


def test_a_config_that_records_nothing_or_too_much_is_refused():
    with pytest.raises(ValueError, match=r'jacobian_posterior: no_samples_MCMC = 80 with period 81 records no step'):
        jacobian_posterior_options({**BASE, 'jacobian_posterior': {'period': 81}})
    big = {'no_samples_MCMC': 2 ** 31, 'log_period_MCMC': 1, 'no_chains': 2}
    with pytest.raises(ValueError, match='jacobian_posterior.*at most 2147483647'):
        jacobian_posterior_options({**big, 'jacobian_posterior': True})
    with pytest.raises(ValueError, match='jacobian_posterior.*2147483648 records'):
        jacobian_posterior_options({**big, 'jacobian_posterior': {'period': 2}})  # 2^30 steps x 2 chains
    assert jacobian_posterior_options({**big, 'no_chains': 1, 'jacobian_posterior': {'period': 2}}) == {'period': 2}
    edge = {'no_samples_MCMC': 2 ** 31 - 1, 'log_period_MCMC': 1, 'no_chains': 1}
    assert jacobian_posterior_options({**edge, 'jacobian_posterior': True}) == {'period': 1}


def test_trainer_refuses_the_config_when_it_is_built(tmp_path):
    from ir_sgmcmc_amd.trainer import Trainer
    config = _config(tmp_path, no_samples_MCMC=4, log_period_MCMC=2, jacobian_posterior={'period': 5})
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    with pytest.raises(ValueError, match='jacobian_posterior'):
        config.init_metrics()
    with pytest.raises(ValueError, match='jacobian_posterior'):
        Trainer(config, dl, losses, tm, rm, [], device='cpu')


def test_init_metrics_names_the_jacobian_posterior_after_the_seg_keys_only_when_on(tmp_path):
    off = _config(tmp_path / 'off').init_metrics()
    assert not [k for k in off if k.startswith('MCMC/jacobian/')]
    keys = [f'MCMC/jacobian/{k}' for k in ('fold_prob_max', 'fold_prob_mean', 'folded_voxels', 'always_folded',
                                           'logJ_std_mean', 'logJ_std_max')]
    assert keys == [f'MCMC/jacobian/{k}' for k in JACOBIAN_METRICS]
    assert _config(tmp_path / 'on', jacobian_posterior=True).init_metrics() == off + keys
    seg = _config(tmp_path / 'seg', label_posterior=True).init_metrics()
    both = _config(tmp_path / 'both', label_posterior=True, jacobian_posterior={'period': 4}).init_metrics()
    assert both == seg + keys and seg[-1] == 'MCMC/seg/ECE'


# ---------------------------------------------------------------- device-free parts of the surface
def test_jacobian_summary_turns_the_columns_into_the_summary():
    s = jacobian_summary([60, 60, 0, 60], [0.25, -0.5, -0.25, 6.0, 0.2], 4)
    assert s == {'records': 4, 'voxels': 60, 'folded_voxels': 60, 'always_folded': 0, 'fold_records': 60, 'fold_prob_max': 0.25,
                 'fold_prob_mean': 0.25, 'logJ_mean_min': -0.5, 'logJ_mean_max': -0.25, 'logJ_std_mean': 0.1, 'logJ_std_max': 0.2}
    inf = float('inf')
    empty = jacobian_summary([0, 0, 0, 0], [-inf, inf, -inf, 0.0, -inf], 4)
    assert empty['voxels'] == 0 and all(math.isnan(empty[k]) for k in ('fold_prob_max', 'fold_prob_mean', 'logJ_mean_min',
                                                                       'logJ_mean_max', 'logJ_std_mean', 'logJ_std_max'))
    folded = jacobian_summary([5, 5, 5, 10], [1.0, inf, -inf, 0.0, -inf], 2)  # every masked voxel folds in every record
    assert folded['fold_prob_max'] == 1.0 and folded['fold_prob_mean'] == 1.0 and math.isnan(folded['logJ_std_mean'])
    assert math.isnan(folded['logJ_mean_min']) and math.isnan(folded['logJ_std_max'])


def test_jacobian_posterior_state_and_refusals():
    jp = JacobianPosterior((3, 4, 5), 'cpu')
    assert tuple(jp.folds.shape) == (3, 4, 5) and jp.folds.dtype == torch.int32
    assert jp.mean.dtype == torch.float32 and jp.m2.dtype == torch.float32 and jp.records == 0
    with pytest.raises(L.IrsError):
        jp.record(torch.zeros(2, 3, 3, 4, 5))  # CPU tensors never reach the library
    assert jp.records == 0
    with pytest.raises(RuntimeError, match='nothing recorded'):
        jp.finalize()
    sd = jp.state_dict()
    assert set(sd) == {'folds', 'mean', 'm2', 'records'}
    sd['records'] = 6
    sd['folds'] = torch.full_like(sd['folds'], 3)
    other = JacobianPosterior((3, 4, 5), 'cpu')
    other.load_state_dict(sd)
    assert other.records == 6 and torch.equal(other.folds, sd['folds'])
    with pytest.raises(ValueError, match='shape'):
        JacobianPosterior((3, 4, 6), 'cpu').load_state_dict(sd)
    assert JacobianPosterior((3, 4, 6), 'cpu').records == 0
    with pytest.raises(ValueError):
        JacobianPosterior((1, 4, 5), 'cpu')
    with pytest.raises(ValueError):
        JacobianPosterior((4, 5), 'cpu')


def test_abi_refusals_without_a_device():
    lib = L.load()
    assert L.IRS_JACOBIAN_WS_BYTES == 1024 * 9 * 8
    p = C.c_void_p(16)  # never dereferenced: every call below is refused before a launch
    big = 1 << 20

    def upd(t=p, Cn=2, D=4, H=4, W=4, folds=p, mean=p, m2=p, before=0):
        return lib.irs_jacobian_posterior_update(t, Cn, D, H, W, folds, mean, m2, before, None)

    def fin(folds=p, mean=p, m2=p, D=4, H=4, W=4, n=4, mask=None, fp=p, lm=p, ls=p, isum=p, fsum=p, ws=p, ws_bytes=big):
        return lib.irs_jacobian_posterior_finalize(folds, mean, m2, D, H, W, n, mask, fp, lm, ls, isum, fsum, ws, ws_bytes, None)

    for kw, msg in ((dict(t=None), 'bad'), (dict(folds=None), 'bad'), (dict(mean=None), 'bad'), (dict(m2=None), 'bad'),
                    (dict(Cn=0), 'bad'), (dict(Cn=9), 'chains'), (dict(D=1), 'bad'), (dict(W=0), 'bad'), (dict(H=-3), 'bad'),
                    (dict(before=-1), 'records_before'), (dict(before=2 ** 31 - 2), 'overflow')):
        assert upd(**kw) != 0, kw
        assert msg in lib.irs_last_error().decode(), (kw, lib.irs_last_error())
    for kw, msg in ((dict(folds=None), 'bad'), (dict(mean=None), 'bad'), (dict(m2=None), 'bad'), (dict(fp=None), 'bad'),
                    (dict(lm=None), 'bad'), (dict(ls=None), 'bad'), (dict(isum=None), 'bad'), (dict(fsum=None), 'bad'),
                    (dict(ws=None), 'bad'), (dict(D=1), 'bad'), (dict(W=0), 'bad'), (dict(n=0), 'n = 0'), (dict(n=-4), 'n = -4'),
                    (dict(ws_bytes=L.IRS_JACOBIAN_WS_BYTES - 1), 'workspace')):
        assert fin(**kw) != 0, kw
        assert msg in lib.irs_last_error().decode(), (kw, lib.irs_last_error())
