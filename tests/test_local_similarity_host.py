"""The local-similarity option's host surface: the known answers the device tests rely on, proved from the numpy restatement
alone (tests/_local_similarity.py), the trainer option, the metric names, the three entry points and what they refuse before
they touch the device.  No GPU needed."""
import copy
import json
import math
import os

import numpy as np
import pytest

from tests import _local_similarity as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def consts(fr=S.UNIT, mr=S.UNIT):
    from ir_sgmcmc_amd.ops import local_similarity_constants
    return local_similarity_constants(fr, mr)


def dyadic(shape, seed):
    """values k / 64: sums and products of a few of them are exact in float32 and float64"""
    return (np.random.default_rng(seed).integers(0, 64, shape) / 64.0).astype(np.float32)


def test_the_constants():
    floor_f, floor_m, c1, c2 = consts((0.0, 2.0), (-1.0, 1.0))
    assert floor_f == (1e-3 * 2.0) ** 2 == floor_m
    assert c1 == (0.01 * 3.0) ** 2 and c2 == (0.03 * 3.0) ** 2
    assert consts() == (1e-6, 1e-6, 1e-4, (0.03) ** 2)
    from ir_sgmcmc_amd._lib import IrsError
    for bad in (((0.0, 0.0), S.UNIT), (S.UNIT, (1.0, 0.0)), ((0.0, math.inf), S.UNIT), (S.UNIT, (math.nan, 1.0))):
        with pytest.raises(IrsError, match='range'):
            consts(*bad)


@pytest.mark.parametrize('r', [1, 2, 4])
def test_identical_images(r):
    f = dyadic((5, 6, 7), 1)
    maps = S.reference_maps(f, f, r, consts())
    assert maps['finite'].all() and not maps['flat'].any()
    assert np.abs(maps['lncc'] - 1.0).max() <= 1e-12 and np.abs(maps['ssim'] - 1.0).max() <= 1e-12
    st = S.reference_stats(maps)
    assert st['n'] == f.size and st['n_flat'] == 0 and st['n_nonfinite'] == 0
    assert st['lncc_mean'] == pytest.approx(1.0, abs=1e-12) and st['ssim_min'] == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize('a,b,sign', [(2.0, 0.5, 1.0), (0.25, 0.0, 1.0), (-1.0, 1.0, -1.0), (-0.5, 2.0, -1.0)])
def test_an_affine_intensity_map_correlates_perfectly(a, b, sign):
    f = dyadic((4, 9, 6), 2)
    m = (a * f + b).astype(np.float32)
    assert (m.astype(np.float64) == a * f.astype(np.float64) + b).all()  # exact: nothing but the window sums rounds
    fr, mr = (0.0, 1.0), (float(m.min()), float(m.max()))
    maps = S.reference_maps(f, m, 2, consts(fr, mr))
    assert not maps['flat'].any()
    assert np.abs(maps['lncc'] - sign).max() <= 1e-12
    assert (maps['ssim'] < 1.0).all()


def test_a_constant_image_is_flat_everywhere():
    f = dyadic((4, 5, 6), 3)
    c = np.full(f.shape, 0.5, np.float32)
    for pair in ((f, c), (c, f), (c, c)):
        maps = S.reference_maps(*pair, 1, consts())
        assert maps['flat'].all() and np.isnan(maps['lncc']).all() and np.isfinite(maps['ssim']).all()
        st = S.reference_stats(maps)
        assert st['n'] == f.size == st['n_flat'] and math.isnan(st['lncc_mean']) and st['lncc_min'] == math.inf
        assert 0.0 < st['ssim_mean'] <= 1.0
    # the variance of a constant window is 0 exactly, not roundoff
    assert (S.reference_maps(c, c, 4, consts())['var_f'] == 0.0).all()
    # an empty mask: means over nothing are NaN, minima +inf
    st = S.reference_stats(S.reference_maps(f, f, 1, consts()), np.zeros(f.shape, bool))
    assert st['n'] == 0 and math.isnan(st['lncc_mean']) and math.isnan(st['ssim_mean'])
    assert st['lncc_min'] == math.inf == st['ssim_min']


def test_a_nonfinite_value_spoils_its_window_only():
    f, m = S.noise_pair((9, 8, 7), 1, seed=4)
    f, m = f[0, 0], m[0, 0]
    clean = S.reference_maps(f, m, 2, consts())
    f2, m2 = f.copy(), m.copy()
    f2[4, 4, 3], m2[0, 0, 0], m2[8, 7, 6] = np.nan, np.inf, -np.inf
    maps = S.reference_maps(f2, m2, 2, consts())
    want = np.zeros(f.shape, bool)
    want[2:7, 2:7, 1:6] = True  # interior: the 5^3 box
    want[:3, :3, :3] = True     # a corner: the clamped window reaches it from 3^3 voxels
    want[6:, 5:, 4:] = True
    assert (maps['finite'] == ~want).all()
    assert np.isnan(maps['lncc'][want]).all() and np.isnan(maps['ssim'][want]).all()
    assert (maps['lncc'][~want] == clean['lncc'][~want]).all() and (maps['ssim'][~want] == clean['ssim'][~want]).all()
    mask = S.random_mask(f.shape, 5)
    st = S.reference_stats(maps, mask)
    assert st['n_nonfinite'] == int((want & mask).sum()) and st['n'] == int((~want & mask).sum())


@pytest.mark.parametrize('shape,r', [((1, 1, 3), 4), ((2, 3, 5), 2), ((6, 7, 9), 1), ((5, 4, 11), 4)])
def test_the_window_is_avg_pool3d_of_the_replicate_padded_volume(shape, r):
    import torch
    import torch.nn.functional as F
    x = np.random.default_rng(6).random(shape)
    n = (2 * r + 1) ** 3
    # F.pad replicates at most the volume's own extent per call: one voxel at a time
    t = torch.from_numpy(x)[None, None]
    for _ in range(r):
        t = F.pad(t, (1, 1, 1, 1, 1, 1), mode='replicate')
    pooled = F.avg_pool3d(t, 2 * r + 1, stride=1)[0, 0].numpy()
    got = S.box_sum(x, r) / n
    assert got.shape == tuple(shape) and np.abs(got - pooled).max() <= 1e-14
    assert t.dtype == torch.float64


# ---------------------------------------------------------------- the option
BASE = {'log_period_MCMC': 4, 'no_samples_MCMC': 8, 'no_chains': 2}


def test_options_helper_parses():
    from ir_sgmcmc_amd.diagnostics import local_similarity_options
    opt = lambda v: local_similarity_options({**BASE, 'local_similarity': v})
    assert local_similarity_options(BASE) is None and opt(False) is None and opt(None) is None
    assert opt(True) == {'period': 4, 'radius': 2, 'save': True} == opt({})
    assert opt({'radius': 4}) == {'period': 4, 'radius': 4, 'save': True}
    assert opt({'period': 3, 'save': False, 'radius': 1}) == {'period': 3, 'radius': 1, 'save': False}


@pytest.mark.parametrize('bad', [1, 'yes', [2], {'r': 2}, {'radius': 2, 'every': 2}, {'radius': 0}, {'radius': 5}, {'radius': 2.0},
                                 {'radius': True}, {'radius': '2'}, {'period': 0}, {'period': -3}, {'period': 2.5}, {'period': True},
                                 {'period': None}, {'period': 9}, {'save': 1}, {'save': 'yes'}, {'save': None}])
def test_options_helper_rejects(bad):
    from ir_sgmcmc_amd.diagnostics import local_similarity_options
    with pytest.raises(ValueError, match='trainer.local_similarity'):
        local_similarity_options({**BASE, 'local_similarity': bad})


def test_options_helper_rejects_more_records_than_the_count_holds():
    from ir_sgmcmc_amd.diagnostics import local_similarity_options
    with pytest.raises(ValueError, match='trainer.local_similarity'):
        local_similarity_options({'log_period_MCMC': 1, 'no_samples_MCMC': 2 ** 30, 'no_chains': 2, 'local_similarity': True})


def _names(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer'].update(save_dir=str(tmp_path), **trainer_over)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    return config, config.init_metrics()


def test_init_metrics_has_the_local_similarity_keys_exactly_when_the_option_is_on(tmp_path):
    config, off = _names(tmp_path)
    assert off == _names(tmp_path, local_similarity=False)[1] and not any('local_similarity' in k for k in off)
    _, on = _names(tmp_path, local_similarity={'radius': 1})
    C = config['trainer']['no_chains']
    prefixes = ['VI/train/local_similarity'] + [f'MCMC/chain_{i}/local_similarity' for i in range(C)] + ['MCMC/local_similarity_of_mean']
    added = [f'{p}/{k}' for p in prefixes for k in ('LNCC', 'LNCC_min', 'SSIM')]
    assert sorted(on) == sorted(off + added) and len(set(on)) == len(on)
    assert [k for k in on if 'local_similarity' not in k] == off  # everything else, in today's order
    assert _names(tmp_path, local_similarity=True)[1] == on
    with pytest.raises(ValueError, match='trainer.local_similarity'):
        _names(tmp_path, local_similarity={'radius': 5})


# ---------------------------------------------------------------- the entry points
NEW = ('irs_local_similarity', 'irs_local_similarity_update', 'irs_local_similarity_finalize')


def test_the_three_symbols_are_declared_bound_and_exported():
    import re
    import subprocess

    from ir_sgmcmc_amd import _lib as L
    header = open(os.path.join(ROOT, 'include', 'irsgmcmc.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(irs_local[a-z0-9_]*)\s*\(', code))
    assert declared == set(NEW) == {k for k in L.SIGNATURES if k.startswith('irs_local')}
    lib = L.load()
    assert all(hasattr(lib, name) for name in NEW)
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NEW) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name, value in (('IRS_LOCAL_MAX_RADIUS', 4), ('IRS_LOCAL_STATS', 7), ('IRS_LOCAL_MAX_BLOCKS', 1024),
                        ('IRS_LOCAL_MAP_SUMMARY_INTS', 2), ('IRS_LOCAL_MAP_SUMMARY_FLOATS', 3)):
        assert re.search(rf'#define {name} {value}\b', header) and getattr(L, name) == value
    assert L.IRS_LOCAL_WS_BYTES == L.IRS_MAX_CHAINS * 1024 * 7 * 8 and L.IRS_LOCAL_MAP_WS_BYTES == 1024 * 5 * 8


def test_the_python_surface_and_cpu_tensors():
    import inspect

    import torch

    from ir_sgmcmc_amd import _lib as L
    from ir_sgmcmc_amd import ops
    from ir_sgmcmc_amd.utils import calc_local_similarity
    assert list(inspect.signature(ops.local_similarity).parameters) == ['fixed', 'moving', 'mask', 'radius', 'fixed_range',
                                                                        'moving_range', 'want']
    assert list(inspect.signature(calc_local_similarity).parameters)[:4] == ['fixed', 'moving', 'mask', 'radius']
    assert inspect.signature(ops.local_similarity).parameters['radius'].default == 2
    assert ops.LOCAL_COLUMNS == S.COLUMNS and len(ops.LOCAL_COLUMNS) == L.IRS_LOCAL_STATS
    im = torch.zeros(1, 1, 4, 4, 4)
    with pytest.raises(L.IrsError):
        ops.local_similarity(im, im, fixed_range=S.UNIT, moving_range=S.UNIT)
    with pytest.raises(L.IrsError):
        ops.local_similarity_update(im, torch.zeros(4, 4, 4), torch.zeros(4, 4, 4), torch.zeros(4, 4, 4, dtype=torch.int32), 0)
    with pytest.raises(L.IrsError):
        ops.local_similarity_finalize(torch.zeros(4, 4, 4), torch.zeros(4, 4, 4), torch.zeros(4, 4, 4, dtype=torch.int32))


def test_arguments_are_validated_on_the_host():
    """everything the three entry points refuse before they touch the device: one fake non-null pointer stands for every array"""
    import ctypes as C

    from ir_sgmcmc_amd import _lib as L
    lib = L.load()
    p = C.c_void_p(256)
    inf, nan = float('inf'), float('nan')

    def sim(fixed=p, Cf=1, moving=p, Cn=2, dims=(4, 4, 4), radius=2, k=(1e-6, 1e-6, 1e-4, 9e-4), stats=p, ws=p,
            ws_bytes=L.IRS_LOCAL_WS_BYTES):
        return lib.irs_local_similarity(fixed, Cf, moving, Cn, None, *dims, radius, *k, None, None, stats, ws, ws_bytes, None)
    cases = [(dict(fixed=None), b'bad arguments'), (dict(moving=None), b'bad arguments'), (dict(stats=None), b'bad arguments'),
             (dict(ws=None), b'bad arguments'), (dict(Cn=0), b'chains'), (dict(Cn=L.IRS_MAX_CHAINS + 1), b'chains'),
             (dict(Cf=3), b'1 or 2'), (dict(Cf=0), b'1 or 2'), (dict(radius=0), b'radius'), (dict(radius=5), b'radius'),
             (dict(radius=-1), b'radius'), (dict(dims=(0, 4, 4)), b'dims'), (dict(dims=(4, 4, -1)), b'dims'),
             (dict(dims=(1024, 1024, 1024)), b'2^30'), (dict(ws_bytes=0), b'workspace'), (dict(ws_bytes=2 * 7 * 8 - 1), b'workspace')]
    for j, name in enumerate((b'floor_f', b'floor_m', b'c1', b'c2')):
        for bad in (0.0, -1.0, inf, nan):
            k = [1e-6, 1e-6, 1e-4, 9e-4]
            k[j] = bad
            cases.append((dict(k=tuple(k)), name))
    for kw, msg in cases:
        assert sim(**kw) != 0, kw
        assert msg in lib.irs_last_error(), (kw, lib.irs_last_error())

    def update(lncc=p, Cn=2, dims=(4, 4, 4), mean=p, low=p, count=p, before=0):
        return lib.irs_local_similarity_update(lncc, Cn, *dims, mean, low, count, before, None)
    for kw, msg in ((dict(lncc=None), b'bad arguments'), (dict(mean=None), b'bad arguments'), (dict(low=None), b'bad arguments'),
                    (dict(count=None), b'bad arguments'), (dict(Cn=0), b'chains'), (dict(Cn=L.IRS_MAX_CHAINS + 1), b'chains'),
                    (dict(dims=(4, 0, 4)), b'dims'), (dict(dims=(1024, 1024, 1024)), b'2^30'), (dict(before=-1), b'records_before'),
                    (dict(before=2 ** 31 - 2), b'overflow')):
        assert update(**kw) != 0, kw
        assert msg in lib.irs_last_error(), (kw, lib.irs_last_error())

    def finalize(mean=p, low=p, count=p, dims=(4, 4, 4), isum=p, fsum=p, ws=p, ws_bytes=L.IRS_LOCAL_MAP_WS_BYTES):
        return lib.irs_local_similarity_finalize(mean, low, count, None, *dims, isum, fsum, ws, ws_bytes, None)
    for kw, msg in ((dict(mean=None), b'bad arguments'), (dict(low=None), b'bad arguments'), (dict(count=None), b'bad arguments'),
                    (dict(isum=None), b'bad arguments'), (dict(fsum=None), b'bad arguments'), (dict(ws=None), b'bad arguments'),
                    (dict(dims=(4, 4, 0)), b'dims'), (dict(dims=(1024, 1024, 1024)), b'2^30'),
                    (dict(ws_bytes=L.IRS_LOCAL_MAP_WS_BYTES - 1), b'workspace')):
        assert finalize(**kw) != 0, kw
        assert msg in lib.irs_last_error(), (kw, lib.irs_last_error())
