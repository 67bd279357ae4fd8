"""Displacement covariance posterior, host side: the hand-checked cases of the definitions against the numpy restatement, the
forward bound and the tolerances the device is held to (checked here with float32 numpy on the GPU test's own inputs), the
5-sweep Jacobi iteration against numpy.linalg.eigh, the config option and its refusals, the metric names, and the parts of the
surface that need no device."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.diagnostics import (COVARIANCE_METRICS, COVARIANCE_OPTION_KEYS, DisplacementCovariance, covariance_summary,
                                       displacement_covariance_options)
from tests._displacement_covariance import (CASES, HAND_FA, HAND_STD, RECIPES, case_seed, check_maps, covariance_np,
                                            default_scale, draw_records, eigh_desc, finalize_np, hand_checked_records, jacobi_np,
                                            matrices, summary_np, welford_np)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {'no_samples_MCMC': 80, 'log_period_MCMC': 10, 'no_chains': 2}
FLOAT_KEYS = ('std_major_mean', 'std_major_max', 'std_total_mean', 'anisotropy_mean', 'anisotropy_max', 'dir_x', 'dir_y', 'dir_z')


def _config(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['trainer'].update(trainer_over)
    return ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize('rotate', [False, True])
def test_hand_checked_case_of_the_restatement(rotate):
    ref = covariance_np(hand_checked_records(rotate=rotate), scale=(1, 1, 1))
    assert np.abs(ref['mean']).max() <= 1e-7
    want = np.diag([8 / 3, 2 / 3, 0.0])
    if rotate:
        r = math.sqrt(0.5)
        Q = np.array([[r, -r, 0], [r, r, 0], [0, 0, 1]])
        want = Q @ want @ Q.T
    assert np.abs(ref['S'] - want).max() <= 1e-6  # sqrt(1/2) in float32
    for i in range(3):
        assert np.abs(ref['std'][i] - HAND_STD[i]).max() <= 1e-6
    d = (math.sqrt(0.5), math.sqrt(0.5), 0.0) if rotate else (1.0, 0.0, 0.0)
    for i in range(3):
        assert np.abs(ref['direction'][i] - d[i]).max() <= 1e-6
    assert np.abs(ref['anisotropy'] - HAND_FA).max() <= 1e-6 and round(HAND_FA, 6) == 0.874475
    s = ref['summary']
    assert (s['records'], s['voxels'], s['nonfinite_voxels']) == (4, 60, 0)
    assert s['std_major_mean'] == pytest.approx(HAND_STD[0], abs=1e-6) and s['std_major_max'] == pytest.approx(HAND_STD[0], abs=1e-6)
    assert s['std_total_mean'] == pytest.approx(math.sqrt(10 / 3), abs=1e-6)
    assert s['anisotropy_mean'] == pytest.approx(HAND_FA, abs=1e-6) and s['dir_z'] == 0.0
    assert s['dir_x'] == pytest.approx(d[0], abs=1e-6) and s['dir_y'] == pytest.approx(d[1], abs=1e-6)
    # and the finalize's own arithmetic (float32 state, Jacobi) on it
    m32, M32 = welford_np(hand_checked_records(rotate=rotate), np.float32)[:2]
    check_maps(ref, *finalize_np(m32, M32, 4, (1, 1, 1)))


def test_one_record_gives_zero_everywhere_and_nan_propagates():
    rec = draw_records('anisotropic', 1, (3, 4, 5), 1)
    ref = covariance_np(rec)
    assert np.array_equal(ref['mean'], rec[0].astype(np.float64)) and not ref['M'].any()
    assert not ref['std'].any() and not ref['direction'].any() and not ref['anisotropy'].any()
    std, d, fa = finalize_np(*welford_np(rec, np.float32)[:2], 1, default_scale((3, 4, 5)))
    assert not std.any() and not d.any() and not fa.any()
    rec = draw_records('anisotropic', 4, (3, 4, 5), 2)
    rec[1, 2, 1, 2, 3] = np.nan
    rec[3, 0, 0, 0, 0] = np.inf
    ref = covariance_np(rec, mask=np.ones((3, 4, 5), dtype=bool))
    assert (~ref['finite']).sum() == 2 and ref['summary']['nonfinite_voxels'] == 2 and ref['summary']['voxels'] == 60
    m32, M32 = welford_np(rec, np.float32)[:2]
    assert np.array_equal(np.isfinite(m32).all(axis=0) & np.isfinite(M32).all(axis=0), ref['finite'])
    check_maps(ref, *finalize_np(m32, M32, 4, ref['scale']))
    empty = summary_np(4, ref['std'], ref['direction'], ref['anisotropy'], np.zeros((3, 4, 5), dtype=bool))
    assert empty['voxels'] == 0 and all(math.isnan(empty[k]) for k in FLOAT_KEYS)


@pytest.mark.parametrize('recipe', RECIPES)
@pytest.mark.parametrize('C,steps,shape', CASES)
def test_the_bound_is_real_on_the_inputs_of_the_gpu_test(C, steps, shape, recipe):
    """a float32 evaluation of the state in the kernel's operation order stays within E of the float64 one; the finalize's
    arithmetic on that state stays inside every tolerance the device is held to; and the conditions on the inputs hold: at
    most 0.5 % of the voxels have a relative gap below 0.05 (anisotropic recipe), none is left out of the FA comparison"""
    n = C * steps
    rec = draw_records(recipe, n, shape, case_seed(C, steps, shape, recipe))
    ref = covariance_np(rec)
    m32, M32 = welford_np(rec, np.float32)[:2]
    assert m32.dtype == np.float32 and M32.dtype == np.float32
    dS = matrices(M32, n, ref['scale']) - ref['S']
    err = np.sqrt((dS ** 2).sum(axis=(-1, -2)))
    assert (err <= ref['E']).all(), float((err / np.maximum(ref['E'], 1e-300)).max())
    if n >= 2:
        assert (ref['E'] > 0).all()
    std, d, fa = finalize_np(m32, M32, n, ref['scale'])
    check_maps(ref, std, d, fa, compare_eigenvector=recipe == 'anisotropic', all_fa=n >= 2)
    if recipe == 'anisotropic' and n >= 8 and min(shape) >= 5:  # the draw is what it says: spreads near 3 : 2 : 1
        ratio = ref['std'][0].mean() / ref['std'][2].mean()
        assert 2.0 <= ratio <= 6.0, ratio


def _adversarial(rng, count):
    """sample covariances of 2-40 anisotropic records, isotropic + 1e-9 noise, rank one, rank one + 1e-6 I, rank one * 1e+-20"""
    out = []
    for n in (2, 3, 5, 10, 40):
        x = rng.standard_normal((count, n, 3)) * np.array([3.0, 2.0, 1.0])
        x = x - x.mean(axis=1, keepdims=True)
        out.append(np.einsum('vka,vkb->vab', x, x) / (n - 1))
    eye = np.eye(3)
    noise = rng.standard_normal((count, 3, 3)) * 1e-9
    out.append(eye + (noise + noise.transpose(0, 2, 1)) / 2)
    v = rng.standard_normal((count, 3))
    one = np.einsum('va,vb->vab', v, v)
    out += [one, one + 1e-6 * eye, one * 1e20, one * 1e-20, np.zeros((4, 3, 3)), np.broadcast_to(eye, (4, 3, 3)).copy()]
    return np.concatenate(out)


def test_five_jacobi_sweeps_match_eigh():
    rng = np.random.default_rng(5)
    mats = [_adversarial(rng, 20000)]
    for recipe in RECIPES:
        for C_, steps, shape in CASES[:7]:
            rec = draw_records(recipe, C_ * steps, shape, case_seed(C_, steps, shape, recipe))
            mats.append(covariance_np(rec)['S'].reshape(-1, 3, 3))
    S = np.concatenate(mats)
    normS = np.sqrt((S ** 2).sum(axis=(1, 2)))
    lam, V, off = jacobi_np(S)
    want, _ = eigh_desc(S)
    figures = {'matrices': len(S), 'off-diagonal / |S|_F': float((off / np.maximum(normS, 1e-300)).max()),
               'eigenvalue error / |S|_F': float((np.abs(lam - want).max(axis=1) / np.maximum(normS, 1e-300)).max())}
    print(figures)
    assert (off <= 2e-16 * normS).all()  # the figure four sweeps reach, with one sweep spare
    assert (np.abs(lam - want) <= 2.6e-15 * normS[:, None]).all()
    # the vectors are orthonormal and diagonalise S
    assert np.abs(np.einsum('vab,vac->vbc', V, V) - np.eye(3)).max() <= 1e-14
    res = np.einsum('vab,vbc->vac', S, V) - V * lam[:, None, :]
    assert (np.sqrt((res ** 2).sum(axis=(1, 2))) <= 1e-14 * normS + 1e-300).all()
    # three sweeps are not enough: the fixed count is not slack
    _, _, off3 = jacobi_np(S, sweeps=3)
    assert (off3 / np.maximum(normS, 1e-300)).max() > 1e-12


# ---------------------------------------------------------------- the config option
def test_option_values():
    assert COVARIANCE_OPTION_KEYS == ('period',)
    assert displacement_covariance_options(BASE) is None
    for off in (False, None):
        assert displacement_covariance_options({**BASE, 'displacement_covariance': off}) is None
    assert displacement_covariance_options({**BASE, 'displacement_covariance': True}) == {'period': 10}
    assert displacement_covariance_options({**BASE, 'displacement_covariance': {}}) == {'period': 10}
    assert displacement_covariance_options({**BASE, 'displacement_covariance': {'period': 3}}) == {'period': 3}
    assert displacement_covariance_options({**BASE, 'displacement_covariance': {'period': 80}}) == {'period': 80}


@pytest.mark.parametrize('opt', [{'period': 0}, {'period': -2}, {'period': 2.5}, {'period': 2.0}, {'period': '2'},
                                 {'period': True}, {'period': None}, {'periods': 2}, {'period': 2, 'maps': True},
                                 {'scale': 1.0}, 'yes', 1, [2]])
def test_option_refusals(opt):
    with pytest.raises(ValueError, match='displacement_covariance'):
        displacement_covariance_options({**BASE, 'displacement_covariance': opt})


def test_a_config_that_records_nothing_or_too_much_is_refused():
    with pytest.raises(ValueError, match=r'displacement_covariance: no_samples_MCMC = 80 with period 81 records no step'):
        displacement_covariance_options({**BASE, 'displacement_covariance': {'period': 81}})
    big = {'no_samples_MCMC': 2 ** 31, 'log_period_MCMC': 1, 'no_chains': 2}
    with pytest.raises(ValueError, match='displacement_covariance.*at most 2147483647'):
        displacement_covariance_options({**big, 'displacement_covariance': True})
    with pytest.raises(ValueError, match='displacement_covariance.*2147483648 records'):
        displacement_covariance_options({**big, 'displacement_covariance': {'period': 2}})  # 2^30 steps x 2 chains
    assert displacement_covariance_options({**big, 'no_chains': 1, 'displacement_covariance': {'period': 2}}) == {'period': 2}


def test_trainer_refuses_the_config_when_it_is_built(tmp_path):
    from ir_sgmcmc_amd.trainer import Trainer
    config = _config(tmp_path, no_samples_MCMC=4, log_period_MCMC=2, displacement_covariance={'period': 5})
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    with pytest.raises(ValueError, match='displacement_covariance'):
        config.init_metrics()
    with pytest.raises(ValueError, match='displacement_covariance'):
        Trainer(config, dl, losses, tm, rm, [], device='cpu')


def test_init_metrics_names_the_covariance_after_the_jacobian_keys_only_when_on(tmp_path):
    off = _config(tmp_path / 'off').init_metrics()
    assert not [k for k in off if k.startswith('MCMC/covariance/')]
    keys = [f'MCMC/covariance/{k}' for k in FLOAT_KEYS]
    assert keys == [f'MCMC/covariance/{k}' for k in COVARIANCE_METRICS]
    assert _config(tmp_path / 'on', displacement_covariance=True).init_metrics() == off + keys
    jac = _config(tmp_path / 'jac', jacobian_posterior=True).init_metrics()
    both = _config(tmp_path / 'both', jacobian_posterior=True, displacement_covariance={'period': 4}).init_metrics()
    assert both == jac + keys and jac[-1] == 'MCMC/jacobian/logJ_std_max'


# ---------------------------------------------------------------- device-free parts of the surface
def test_covariance_summary_turns_the_columns_into_the_summary():
    s = covariance_summary([60, 10], [100.0, 3.0, 150.0, 25.0, 0.9, 30.0, 15.0, 5.0], 4)
    assert s == {'records': 4, 'voxels': 60, 'nonfinite_voxels': 10, 'std_major_mean': 2.0, 'std_major_max': 3.0,
                 'std_total_mean': 3.0, 'anisotropy_mean': 0.5, 'anisotropy_max': 0.9, 'dir_x': 0.6, 'dir_y': 0.3, 'dir_z': 0.1}
    inf = float('inf')
    empty = covariance_summary([0, 0], [0.0, -inf, 0.0, 0.0, -inf, 0.0, 0.0, 0.0], 4)
    assert empty['voxels'] == 0 and empty['records'] == 4 and all(math.isnan(empty[k]) for k in FLOAT_KEYS)
    bad = covariance_summary([5, 5], [0.0, -inf, 0.0, 0.0, -inf, 0.0, 0.0, 0.0], 2)  # no masked voxel is finite
    assert bad['voxels'] == 5 and bad['nonfinite_voxels'] == 5 and all(math.isnan(bad[k]) for k in FLOAT_KEYS)


def test_displacement_covariance_state_and_refusals():
    dc = DisplacementCovariance((3, 4, 5), 'cpu')
    assert tuple(dc.mean.shape) == (3, 3, 4, 5) and tuple(dc.comoment.shape) == (6, 3, 4, 5)
    assert dc.mean.dtype == torch.float32 and dc.comoment.dtype == torch.float32 and dc.records == 0
    assert dc.default_scale() == (2.0, 1.5, 1.0) == default_scale((3, 4, 5))
    with pytest.raises(L.IrsError):
        dc.record(torch.zeros(2, 3, 3, 4, 5))  # CPU tensors never reach the library
    assert dc.records == 0
    with pytest.raises(RuntimeError, match='nothing recorded'):
        dc.finalize()
    with pytest.raises(RuntimeError, match='nothing recorded'):
        dc.covariance()
    sd = dc.state_dict()
    assert set(sd) == {'mean', 'comoment', 'records'}
    sd['records'] = 6
    sd['comoment'] = torch.full_like(sd['comoment'], 3.0)
    other = DisplacementCovariance((3, 4, 5), 'cpu')
    other.load_state_dict(sd)
    assert other.records == 6 and torch.equal(other.comoment, sd['comoment'])
    assert torch.equal(other.covariance(), sd['comoment'] / 5)
    with pytest.raises(ValueError, match='shape'):
        DisplacementCovariance((3, 4, 6), 'cpu').load_state_dict(sd)
    with pytest.raises(ValueError):
        DisplacementCovariance((1, 4, 5), 'cpu')
    with pytest.raises(ValueError):
        DisplacementCovariance((4, 5), 'cpu')


def test_abi_refusals_without_a_device():
    lib = L.load()
    assert (L.IRS_COVARIANCE_SUMMARY_INTS, L.IRS_COVARIANCE_SUMMARY_FLOATS) == (2, 8)
    assert L.IRS_COVARIANCE_WS_BYTES == 1024 * 10 * 8
    p = C.c_void_p(16)  # never dereferenced: every call below is refused before a launch
    big = 1 << 20
    good = (C.c_float * 3)(1.0, 1.0, 1.0)

    def upd(x=p, Cn=2, D=4, H=4, W=4, mean=p, com=p, before=0):
        return lib.irs_displacement_covariance_update(x, Cn, D, H, W, mean, com, before, None)

    def fin(mean=p, com=p, D=4, H=4, W=4, n=4, scale=good, mask=None, std=p, d=p, fa=p, isum=p, fsum=p, ws=p, ws_bytes=big):
        return lib.irs_displacement_covariance_finalize(mean, com, D, H, W, n, scale, mask, std, d, fa, isum, fsum, ws, ws_bytes, None)

    for kw, msg in ((dict(x=None), 'bad'), (dict(mean=None), 'bad'), (dict(com=None), 'bad'), (dict(Cn=0), 'bad'),
                    (dict(Cn=9), 'chains'), (dict(D=1), 'bad'), (dict(W=0), 'bad'), (dict(H=-3), 'bad'),
                    (dict(before=-1), 'records_before'), (dict(before=2 ** 31 - 2), 'overflow')):
        assert upd(**kw) != 0, kw
        assert msg in lib.irs_last_error().decode(), (kw, lib.irs_last_error())
    scales = [(C.c_float * 3)(*s) for s in ((0.0, 1, 1), (1, -1.0, 1), (1, 1, float('nan')), (float('inf'), 1, 1))]
    for kw, msg in ((dict(mean=None), 'bad'), (dict(com=None), 'bad'), (dict(scale=None), 'bad'), (dict(std=None), 'bad'),
                    (dict(d=None), 'bad'), (dict(fa=None), 'bad'), (dict(isum=None), 'bad'), (dict(fsum=None), 'bad'),
                    (dict(ws=None), 'bad'), (dict(D=1), 'bad'), (dict(W=0), 'bad'), (dict(n=0), 'n = 0'), (dict(n=-4), 'n = -4'),
                    (dict(ws_bytes=L.IRS_COVARIANCE_WS_BYTES - 1), 'workspace'), *((dict(scale=s), 'scale') for s in scales)):
        assert fin(**kw) != 0, kw
        assert msg in lib.irs_last_error().decode(), (kw, lib.irs_last_error())
