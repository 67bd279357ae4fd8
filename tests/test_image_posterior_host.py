"""Image posterior, host side: the numpy restatement against a float64 two-pass evaluation and against the oracle's sampler, the
band of the float32 recurrence on the record sets of the GPU test (measured, printed and held to the stored value), the config
option and its refusals, load_volume, the metric names, the refusals of the C ABI (which happen before any launch) and the parts
of the surface that need no device."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import image_posterior as IP
from ir_sgmcmc_amd.diagnostics import (IMAGE_METRICS, IMAGE_Z_METRICS, ImagePosterior, image_posterior_metric_names,
                                       image_posterior_names, image_posterior_options, image_summary)
from ir_sgmcmc_amd.utils.imageio import write_nifti
from tests import _exact_cases as X
from tests import _image_posterior as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {'no_samples_MCMC': 80, 'log_period_MCMC': 10, 'no_chains': 2}
DEFAULTS = {'period': 10, 'volumes': (), 'reference': True, 'std_floor': None, 'save': True}


def _config(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['trainer'].update(trainer_over)
    return ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_restated_sampler_is_the_oracles_on_the_exact_cases(dims):
    """on the dyadic cases float32 and float64 agree bit for bit, so the restated taps must reproduce the oracle's warp exactly"""
    case = X.warp_case(dims, False)
    t = (X.identity(dims) + case.d_last).numpy()
    want = X.warp_reference(case, torch.float64)[0][:, 0].numpy()
    tp = R.taps(t, dims)
    assert np.array_equal(R.sample32(case.im.numpy(), tp).astype(np.float64), want)
    assert np.array_equal(R.sample64(case.im.numpy(), tp), want)
    # the exact cases sit on voxel centres and borders: some taps read with weight 0
    off, w = tp
    assert (w == 0).any() and (off >= 0).all() and (off < np.prod(dims)).all()


def test_restated_sampler_on_random_positions_against_the_oracle():
    from oracle import ops as O
    shape = (5, 7, 9)
    t = R.random_transformation(shape, 2, 11)
    vol = R.random_volumes(shape, 1, 12)
    want = O.warp_trilinear(torch.from_numpy(vol).double().expand(2, -1, -1, -1, -1), torch.from_numpy(t).double())[:, 0].numpy()
    tp = R.taps(t, shape)
    # the positions are float32 on both sides; the oracle unnormalises them in float64, the kernel in float32: 3 roundings of
    # a coordinate <= n + 2, times the largest slope of the image, 10 per voxel
    assert np.abs(R.sample64(vol, tp) - want).max() <= 3 * 2.0 ** -24 * 12 * 10 * 3
    assert np.abs(R.sample32(vol, tp).astype(np.float64) - R.sample64(vol, tp)).max() <= 8 * 2.0 ** -24 * 10
    coords = X.voxel_coordinates(torch.from_numpy(t), shape)
    for raw, n in zip(coords, X.axis_sizes(shape)):
        assert float(raw.min()) == pytest.approx(-3, abs=1e-5) and float(raw.max()) == pytest.approx(n + 2, abs=1e-5)


def test_fold_of_a_hand_checked_case():
    rec = np.array([[1.0, 2.0], [3.0, 2.0], [8.0, 2.0]], np.float32)
    mean, m2, low, high = R.welford32(rec)
    assert mean.tolist() == [4.0, 2.0] and m2.tolist() == [26.0, 0.0] and low.tolist() == [1.0, 2.0] and high.tolist() == [8.0, 2.0]
    m64, v64, lo64, hi64 = R.two_pass(rec)
    assert m64.tolist() == [4.0, 2.0] and v64.tolist() == [13.0, 0.0] and lo64.tolist() == [1.0, 2.0] and hi64.tolist() == [8.0, 2.0]
    # the fold continues from a state, and its first record overwrites whatever the state held
    part = R.welford32(rec[:1])
    cont = R.welford32(rec[1:], part, 1)
    assert all(np.array_equal(a, b) for a, b in zip(cont, (mean, m2, low, high)))
    junk = tuple(np.full(2, np.nan, np.float32) for _ in range(4))
    assert all(np.array_equal(a, b) for a, b in zip(R.welford32(rec, junk, 0), (mean, m2, low, high)))
    std, rng, z = R.finalize_np(mean, m2, low, high, 3, reference=np.array([4.0, 5.0], np.float32), std_floor=0.0)
    assert std.tolist() == [np.float32(math.sqrt(13.0)), 0.0] and rng.tolist() == [7.0, 0.0]
    assert z[0] == 0.0 and np.isinf(z[1])
    # a NaN record: the mean is lost for good, the extremes ignore it
    bad = R.welford32(np.array([[1.0], [np.nan], [3.0]], np.float32))
    assert np.isnan(bad[0][0]) and bad[2][0] == 1.0 and bad[3][0] == 3.0
    std, rng, z = R.finalize_np(*bad, 3, reference=np.zeros(1, np.float32), std_floor=1.0)
    assert np.isnan(std[0]) and np.isnan(rng[0]) and np.isnan(z[0])
    ints, floats = R.summary_np(bad[0], std, rng, z)
    assert ints == [1, 1, 0, 0] and floats[:2] == [0.0, 0.0] and floats[2] == -np.inf and floats[5] == -np.inf


def test_restatement_band():
    """the float32 recurrence against the float64 two-pass on exactly the record sets of the GPU test: the measured worst
    errors are printed and the stored band (tests/_image_posterior.py) must hold them without being more than twice as wide"""
    worst_var, worst_mean = 0.0, 0.0
    for shape in R.STEP_SHAPES:
        for C_ in R.STEP_CHAINS:
            volumes, steps = R.step_case(shape, C_)
            records = [[] for _ in range(len(volumes))]
            for t in steps:
                tp = R.taps(t, shape)
                for s, vol in enumerate(volumes):
                    records[s].extend(R.sample32(vol, tp))
                K = len(records[0])
                for rec in records:
                    rec = np.stack(rec)
                    magnitude = float(np.abs(rec).max())
                    mean, m2, low, high = R.welford32(rec)
                    m64, v64, lo64, hi64 = R.two_pass(rec)
                    assert np.array_equal(low, lo64) and np.array_equal(high, hi64)
                    var32 = m2.astype(np.float64) / max(K - 1, 1)
                    worst_var = max(worst_var, float(np.abs(var32 - v64).max()) / magnitude ** 2)
                    frac = float(np.abs(mean - m64).max()) / R.mean_bound(K, magnitude)
                    assert frac <= 1.0, (shape, C_, K, frac)
                    worst_mean = max(worst_mean, frac)
    print(f'image posterior restatement: worst variance error {worst_var:.4e} max|x|^2, worst mean error {worst_mean:.4f} of the bound')
    assert worst_var <= R.VAR_BAND <= 2 * worst_var, (worst_var, R.VAR_BAND)
    assert worst_mean <= R.MEAN_BAND <= 2 * worst_mean, (worst_mean, R.MEAN_BAND)


# ---------------------------------------------------------------- the config option
def test_option_values():
    assert image_posterior_options(BASE) is None
    for off in (False, None):
        assert image_posterior_options({**BASE, 'image_posterior': off}) is None
    assert image_posterior_options({**BASE, 'image_posterior': True}) == DEFAULTS
    assert image_posterior_options({**BASE, 'image_posterior': {}}) == DEFAULTS
    vols = [{'name': 'dose', 'path': 'dose.nii.gz'}, {'name': 'PET_2', 'path': '/data/pet.nii'}]
    got = image_posterior_options({**BASE, 'image_posterior': {'period': 3, 'volumes': vols, 'reference': False, 'std_floor': 0,
                                                               'save': False}})
    assert got == {'period': 3, 'volumes': tuple(vols), 'reference': False, 'std_floor': 0.0, 'save': False}
    assert image_posterior_names(got) == ['moving', 'dose', 'PET_2']
    assert image_posterior_options({**BASE, 'image_posterior': {'std_floor': 2.5}})['std_floor'] == 2.5
    assert image_posterior_options({**BASE, 'image_posterior': {'std_floor': None}})['std_floor'] is None
    seven = [{'name': f'v{i}', 'path': f'{i}.nii'} for i in range(7)]
    assert len(image_posterior_options({**BASE, 'image_posterior': {'volumes': seven}})['volumes']) == 7
    assert image_posterior_options({**BASE, 'image_posterior': {'period': 80}})['period'] == 80


@pytest.mark.parametrize('opt,key', [
    ({'period': 0}, 'period'), ({'period': 2.5}, 'period'), ({'period': True}, 'period'), ({'periods': 2}, 'periods'),
    ({'volume': []}, 'volume'), ({'volumes': 'dose.nii'}, 'volumes'), ({'volumes': [{'name': 'a'}]}, r'volumes\[0\]'),
    ({'volumes': ['a.nii']}, r'volumes\[0\]'), ({'volumes': [{'name': 'a', 'path': 'a', 'unit': 'Gy'}]}, r'volumes\[0\]'),
    ({'volumes': [{'name': 'a b', 'path': 'a'}]}, r'volumes\[0\]\.name'), ({'volumes': [{'name': '', 'path': 'a'}]}, r'volumes\[0\]\.name'),
    ({'volumes': [{'name': 3, 'path': 'a'}]}, r'volumes\[0\]\.name'), ({'volumes': [{'name': 'moving', 'path': 'a'}]}, 'moving'),
    ({'volumes': [{'name': 'a', 'path': 'a'}, {'name': 'a', 'path': 'b'}]}, r'volumes\[1\]\.name.*twice'),
    ({'volumes': [{'name': 'a', 'path': ''}]}, r'volumes\[0\]\.path'), ({'volumes': [{'name': 'a', 'path': 3}]}, r'volumes\[0\]\.path'),
    ({'volumes': [{'name': f'v{i}', 'path': 'a'} for i in range(8)]}, 'volumes: 8 entries, at most 7'),
    ({'reference': 1}, 'reference'), ({'reference': 'fixed'}, 'reference'), ({'save': None}, 'save'), ({'save': 'yes'}, 'save'),
    ({'std_floor': -1e-3}, 'std_floor'), ({'std_floor': float('nan')}, 'std_floor'), ({'std_floor': float('inf')}, 'std_floor'),
    ({'std_floor': '1'}, 'std_floor'), ({'std_floor': True}, 'std_floor'), ('yes', 'must be true, false or'), (1, 'must be true, false or'),
    ([2], 'must be true, false or')])
def test_option_refusals(opt, key):
    with pytest.raises(ValueError, match=rf'trainer\.image_posterior.*{key}'):
        image_posterior_options({**BASE, 'image_posterior': opt})


def test_a_config_that_records_nothing_or_too_much_is_refused():
    with pytest.raises(ValueError, match=r'image_posterior: no_samples_MCMC = 80 with period 81 records no step'):
        image_posterior_options({**BASE, 'image_posterior': {'period': 81}})
    big = {'no_samples_MCMC': 2 ** 31, 'log_period_MCMC': 1, 'no_chains': 2}
    with pytest.raises(ValueError, match='image_posterior.*at most 2147483647'):
        image_posterior_options({**big, 'image_posterior': True})


def test_metric_names(tmp_path):
    off = _config(tmp_path / 'off').init_metrics()
    assert not [k for k in off if k.startswith('MCMC/image/')]
    on = image_posterior_options({**BASE, 'image_posterior': True})
    keys = [f'MCMC/image/moving/{k}' for k in ('std_mean', 'std_max', 'range_max', 'z_rms', 'z_gt2', 'z_gt3')]
    assert image_posterior_metric_names(on) == keys == [f'MCMC/image/moving/{k}' for k in IMAGE_METRICS + IMAGE_Z_METRICS]
    assert _config(tmp_path / 'on', image_posterior=True).init_metrics() == off + keys
    opt = {'volumes': [{'name': 'dose', 'path': 'x'}], 'reference': False}
    names = image_posterior_metric_names(image_posterior_options({**BASE, 'image_posterior': opt}))
    assert names == [f'MCMC/image/{n}/{k}' for n in ('moving', 'dose') for k in IMAGE_METRICS]
    jac = _config(tmp_path / 'jac', jacobian_posterior=True).init_metrics()
    both = _config(tmp_path / 'both', jacobian_posterior=True, image_posterior=True).init_metrics()
    assert both == jac + keys and jac[-1] == 'MCMC/jacobian/logJ_std_max'


def _trainer(config, device='cpu'):
    from ir_sgmcmc_amd.trainer import Trainer
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, losses, tm, rm, [], device=device)


def test_trainer_refuses_the_config_when_it_is_built(tmp_path):
    with pytest.raises(ValueError, match='image_posterior'):
        _trainer(_config(tmp_path / 'a', no_samples_MCMC=4, log_period_MCMC=2, image_posterior={'period': 5}))
    missing = str(tmp_path / 'no_such_dose.nii.gz')
    with pytest.raises(FileNotFoundError, match='no_such_dose'):
        _trainer(_config(tmp_path / 'b', image_posterior={'volumes': [{'name': 'dose', 'path': missing}]}))
    dims = _config(tmp_path / 'c')['data_loader']['args']['dims']
    there = str(tmp_path / 'dose.nii.gz')
    write_nifti(np.zeros(dims, np.float32), there)
    t = _trainer(_config(tmp_path / 'd', image_posterior={'volumes': [{'name': 'dose', 'path': there}]}))
    assert t.image_options['volumes'] == ({'name': 'dose', 'path': there},) and t._image_posterior is None and t.image_summary is None
    off = _trainer(_config(tmp_path / 'e'))
    assert off.image_options is None and off._image_volumes is None and off.image_maps is None


def test_trainer_refuses_extra_volumes_beside_native_resolution(tmp_path, monkeypatch):
    """the extras are read on the registration grid only"""
    from ir_sgmcmc_amd.trainer import trainer as T
    there = str(tmp_path / 'dose.nii.gz')
    write_nifti(np.zeros((4, 4, 4), np.float32), there)
    monkeypatch.setattr(T, 'native_resolution_options', lambda cfg, dl=None: {'period': None, 'save': ()})
    with pytest.raises(ValueError, match=r'image_posterior\.volumes.*native_resolution'):
        _trainer(_config(tmp_path / 'a', image_posterior={'volumes': [{'name': 'dose', 'path': there}]}))
    # the moving image alone is fine beside it
    assert _trainer(_config(tmp_path / 'b', image_posterior=True)).image_options['volumes'] == ()


# ---------------------------------------------------------------- load_volume
class _Loader:
    dims = (4, 5, 6)


def test_load_volume_shape_check_and_round_trip(tmp_path):
    vol = np.random.default_rng(0).normal(50.0, 20.0, (4, 5, 6)).astype(np.float32)
    path = str(tmp_path / 'vol.nii.gz')
    write_nifti(vol, path, (1.0, 2.0, 3.0))
    got = IP.load_volume(path, _Loader())
    assert tuple(got.shape) == (1, 1, 4, 5, 6) and got.dtype == torch.float32 and got.is_contiguous()
    assert np.array_equal(got[0, 0].numpy(), vol)  # intensities as they are
    other = str(tmp_path / 'other.nii.gz')
    write_nifti(np.zeros((4, 5, 7), np.float32), other)
    with pytest.raises(ValueError, match=r'\(4, 5, 7\).*\(4, 5, 6\)'):
        IP.load_volume(other, _Loader())
    with pytest.raises(FileNotFoundError, match='nowhere'):
        IP.load_volume(str(tmp_path / 'nowhere.nii.gz'), _Loader())


def test_load_volume_goes_through_the_data_set_of_a_biobank_loader(tmp_path):
    from ir_sgmcmc_amd.data_loader.datasets import BiobankDataset
    rng = np.random.default_rng(1)
    for sub in ('', 'masks', 'segs'):
        os.makedirs(tmp_path / 'data' / sub, exist_ok=True)
        for name in ('a', 'b'):
            write_nifti(rng.uniform(0, 9, (6, 8, 7)).astype(np.float32), str(tmp_path / 'data' / sub / f'{name}.nii.gz'))
    ds = BiobankDataset((5, 5, 5), str(tmp_path / 'data'))
    loader = type('Loader', (), {'dataset': ds, 'dims': (5, 5, 5)})()
    moving = ds[0][1]['im']
    got = IP.load_volume(str(tmp_path / 'data' / 'b.nii.gz'), loader)
    assert tuple(got.shape) == (1, 1, 5, 5, 5) and torch.equal(got[0], moving)  # the same padding and trilinear resize


# ---------------------------------------------------------------- device-free parts of the surface
def test_image_summary_turns_the_columns_into_the_summary():
    s = image_summary([10, 2, 4, 1], [16.0, 4.0, 1.5, 3.0, 32.0, 3.5], 6, True)
    assert s == {'records': 6, 'voxels': 10, 'nonfinite_voxels': 2, 'mean': 2.0, 'std_mean': 0.5, 'std_max': 1.5, 'range_max': 3.0,
                 'z_rms': 2.0, 'z_max': 3.5, 'z_gt2': 0.5, 'z_gt3': 0.125}
    plain = image_summary([10, 2, 0, 0], [16.0, 4.0, 1.5, 3.0, math.nan, math.nan], 6, False)
    assert plain == {k: v for k, v in s.items() if not k.startswith('z_')}
    inf = float('inf')
    empty = image_summary([0, 0, 0, 0], [0.0, 0.0, -inf, -inf, 0.0, -inf], 6, True)
    assert empty['voxels'] == 0 and all(math.isnan(empty[k]) for k in ('mean', 'std_mean', 'std_max', 'range_max', 'z_rms', 'z_max',
                                                                       'z_gt2', 'z_gt3'))


def test_image_posterior_state_and_refusals():
    vols = torch.zeros(3, 1, 3, 4, 5)
    ip = ImagePosterior(vols, ('moving', 'dose', 'pet'), 'cpu')
    assert set(ip.state) == set(IP.STATE_KEYS) and all(tuple(t.shape) == (3, 3, 4, 5) and t.dtype == torch.float32
                                                       for t in ip.state.values())
    with pytest.raises(L.IrsError):
        ip.record(torch.zeros(2, 3, 3, 4, 5))  # CPU tensors never reach the library
    assert ip.records == 0
    with pytest.raises(RuntimeError, match='nothing recorded'):
        ip.finalize()
    sd = ip.state_dict()
    assert set(sd) == {'records', 'names', 'dims', *IP.STATE_KEYS} and sd['names'] == ['moving', 'dose', 'pet'] and sd['dims'] == [3, 4, 5]
    sd['records'] = 6
    sd['low'] = torch.full_like(sd['low'], 3)
    other = ImagePosterior(vols, ('moving', 'dose', 'pet'), 'cpu')
    other.load_state_dict(sd)
    assert other.records == 6 and torch.equal(other.state['low'], sd['low'])
    with pytest.raises(ValueError, match='volumes.*does not match'):
        ImagePosterior(vols, ('moving', 'pet', 'dose'), 'cpu').load_state_dict(sd)
    with pytest.raises(ValueError, match='dims.*does not match'):
        ImagePosterior(torch.zeros(3, 1, 3, 4, 6), ('moving', 'dose', 'pet'), 'cpu').load_state_dict(sd)
    for bad_vols, names in ((vols, ('a', 'b')), (vols, ('a', 'a', 'b')), (torch.zeros(3, 2, 3, 4, 5), ('a', 'b', 'c')),
                            (torch.zeros(3, 3, 4, 5), ('a', 'b', 'c'))):
        with pytest.raises(ValueError):
            ImagePosterior(bad_vols, names, 'cpu')
    with pytest.raises(L.IrsError):
        ImagePosterior(torch.zeros(9, 1, 3, 4, 5), [str(i) for i in range(9)], 'cpu')
    for S, dims in ((0, (3, 4, 5)), (9, (3, 4, 5)), (True, (3, 4, 5)), (2, (1, 4, 5)), (2, (4, 5))):
        with pytest.raises(L.IrsError):
            IP.image_posterior_state(S, dims, 'cpu')


def test_python_wrappers_refuse_before_the_library(monkeypatch):
    """shapes, dtypes, index and floor are checked on the host: nothing below may reach the C ABI"""
    monkeypatch.setattr(IP, '_call', lambda *a: pytest.fail('reached the library'))
    state = IP.image_posterior_state(2, (3, 4, 5), 'cpu')
    t = torch.zeros(2, 3, 3, 4, 5)
    vols = torch.zeros(2, 1, 3, 4, 5)
    for kw in (dict(volumes=torch.zeros(2, 1, 3, 4, 6)), dict(volumes=torch.zeros(2, 3, 4, 5)), dict(volumes=torch.zeros(3, 1, 3, 4, 5)),
               dict(volumes=torch.zeros(9, 1, 3, 4, 5)), dict(transformation=torch.zeros(2, 2, 3, 4, 5)),
               dict(state={**state, 'm2': state['m2'].double()}), dict(state={k: v for k, v in state.items() if k != 'high'}),
               dict(state={**state, 'low': state['low'][:1]})):
        with pytest.raises(L.IrsError):
            IP.image_posterior_update(**{'volumes': vols, 'transformation': t, 'state': state, 'records_before': 0, **kw})
    for kw in (dict(index=2), dict(index=-1), dict(index=True), dict(index=0.0), dict(std_floor=-1.0), dict(std_floor=math.nan),
               dict(std_floor=math.inf), dict(reference=torch.zeros(3, 4, 6)), dict(reference=torch.zeros(3, 4, 5).double()),
               dict(mask=torch.zeros(3, 4)), dict(mask=torch.zeros(3, 4, 5)), dict(state={'mean': state['mean']})):
        with pytest.raises(L.IrsError):
            IP.image_posterior_finalize(**{'state': state, 'index': 0, 'n': 2, **kw})


def test_abi_constants_and_refusals_without_a_device():
    lib = L.load()
    assert L.IRS_IMAGE_POSTERIOR_MAX_VOLUMES == 8 == IP.MAX_VOLUMES
    assert L.IRS_IMAGE_POSTERIOR_WS_BYTES == R.WS == 1024 * (len(IP.INT_COLUMNS) + len(IP.FLOAT_COLUMNS)) * 8
    p = C.c_void_p(16)  # never dereferenced: every call below is refused before a launch
    total = 0
    for fn, good, cases in R.abi_refusals(p):
        assert len(good) == len(L.SIGNATURES[fn])
        for cid, replaced, msg in cases:
            rc, err = R.abi_call(lib, fn, good, replaced)
            assert rc != 0 and err == f'{fn}: {msg}', (fn, cid, rc, err)
            total += 1
    assert total == 18 + 19
