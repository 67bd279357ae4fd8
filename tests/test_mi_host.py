"""The float64 restatement of the MI data term (tests/_mi.py) and everything about the feature that needs no device: its gradient
against central finite differences of the definition, sum pmi = n MI, the mistakes its tolerance is there to catch, config parsing,
the refusals of the engine, the trainer and the slab engine, the ABI symbols and the synthetic loader's moving_contrast."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from tests import _mi as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (5, 7, 9)
RANGES = ((0.0, 1.0), (-0.05, 1.05))  # the moving range a little wider than the data: no clamped coordinate, MI is smooth in m


def small_pair(seed=1):
    fixed, moving = M.pair(SHAPE, 1, seed)
    return fixed[0, 0], moving[0, 0]


@pytest.mark.parametrize('bins', [8, 32])
def test_gradient_equals_central_differences(bins):
    """deviation <= 1e-5 max|g| at step 1e-6 (this pair measures 6.7e-8 at max|g| = 8.1 with 8 bins and 7.9e-7 at max|g| = 37 with
    32; the margin is the truncation of the differences).  The differences are taken on the definition with real weights: the Q30 rounding is a
    step function of m, and moves the analytic gradient by 1e-6 only."""
    f, m = small_pair()
    ref = M.reference_one(f, m, None, bins, *RANGES)
    assert ref['inside'].all() and ref['n'] == f.size
    h, m64 = 1e-6, m.astype(np.float64)
    fd = np.zeros(m.size)
    for i in range(m.size):
        mp, mn = m64.copy().reshape(-1), m64.copy().reshape(-1)
        mp[i] += h
        mn[i] -= h
        fd[i] = (M.loss_one(f, mp, None, bins, *RANGES, q_bits=None) - M.loss_one(f, mn, None, bins, *RANGES, q_bits=None)) / (2 * h)
    top = float(np.abs(ref['g']).max())
    dev = float(np.abs(fd - ref['g'].reshape(-1)).max())
    print(f'bins {bins}: max|g| {top:.4g}, deviation {dev:.3g}')
    assert top > 1.0 and dev <= 1e-5 * top


@pytest.mark.parametrize('bins', [8, 32, 64])
def test_pmi_sums_to_n_mi(bins):
    f, m = small_pair(2)
    mask = np.random.default_rng(3).random(SHAPE) < 0.7
    ref = M.reference_one(f, m, mask, bins, (0.0, 1.0), (0.1, 0.9))  # (some coordinates clamped: pmi is defined there too)
    assert ref['n_clipped'] > 0
    # with the weights the histogram received (q_j / 2^30) the identity is exact: 1e-12 relative; the pmi map itself uses the w_j,
    # whose distance from them (at most 2^-31, three times that for q_1) bounds what its sum may miss n MI by
    assert abs(ref['pmi_q_sum'] - ref['n'] * ref['mi']) <= 1e-12 * abs(ref['n'] * ref['mi'])
    total = math.fsum(ref['pmi'].reshape(-1))
    print(f'bins {bins}: sum pmi - n MI = {total - ref["n"] * ref["mi"]:.3g}, bound {ref["pmi_q_bound"]:.3g}')
    assert abs(total - ref['pmi_q_sum']) <= ref['pmi_q_bound']
    assert 0.0 <= ref['mi'] <= math.log(bins) and ref['data_term'] >= 0.0
    assert not ref['g'][~ref['take']].any() and not ref['g'][ref['take'] & ~ref['inside']].any()


def test_histogram_is_exact_and_empty_mask_is_zero():
    f, m = small_pair(4)
    ref = M.reference_one(f, m, None, 16, *RANGES)
    assert int(ref['hist'].sum(dtype=np.uint64)) == ref['n'] << 30
    assert (ref['rows'] == ref['counts_a'].astype(np.uint64) << np.uint64(30)).all()
    none = M.reference_one(f, m, np.zeros(SHAPE, bool), 16, *RANGES)
    assert none['n'] == 0 and none['data_term'] == 0.0 and not none['g'].any() and not none['hist'].any()


@pytest.mark.parametrize('bins', [8, 32])
@pytest.mark.parametrize('mistake', M.MISTAKES)
def test_each_mistake_exceeds_the_tolerance(mistake, bins):
    f, m = small_pair(5)
    ref = M.reference_one(f, m, None, bins, (0.0, 1.0), (0.1, 0.9))
    wrong = M.reference_one(f, m, None, bins, (0.0, 1.0), (0.1, 0.9), mistake=mistake)
    some = ref['tol_g'] > 0
    factor = float((np.abs(wrong['g'] - ref['g'])[some] / ref['tol_g'][some]).max())
    print(f'{mistake}, {bins} bins: {factor:.3g} x the tolerance')
    assert factor > 1000.0


def test_pb_alone_changes_nothing():
    """why the third mistake comes WITH unnormalised weights: the row constant ln p_a cancels while the derivatives sum to zero"""
    f, m = small_pair(5)
    k0, u, _ = M.coords(m.reshape(-1), 0.1, 0.9, 8)
    assert np.abs(M.weight_derivatives(u).sum(axis=0)).max() < 1e-15 and np.abs(M.weights(u).sum(axis=0) - 1.0).max() < 1e-15
    assert k0.min() >= 1 and k0.max() <= 8 - 3


def test_switch_value_and_abi_symbols():
    assert (L.IRS_DATA_GMM_LCC, L.IRS_DATA_SSD, L.IRS_DATA_LNCC, L.IRS_DATA_MI) == (0, 1, 3, 4)
    header = open(os.path.join(ROOT, 'include', 'irsgmcmc.h')).read()
    exports = open(os.path.join(ROOT, 'ir_sgmcmc_amd', 'csrc', 'exports.map')).read()
    assert re.search(r'IRS_DATA_MI = 4\b', header) and 'global: irs_*;' in exports
    for name in ('irs_mi_fwd', 'irs_mi_bwd', 'irs_mi_set'):
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in L.SIGNATURES
    for name, value in (('IRS_MI_STATS', 7), ('IRS_MI_MIN_BINS', 8), ('IRS_MI_MAX_BINS', 64), ('IRS_MI_MAX_BLOCKS', 1024)):
        assert int(re.search(r'#define %s (\d+)' % name, header).group(1)) == value == getattr(L, name)
    assert L.IRS_MI_WS_BYTES == 8 * 64 * 64 * 8 + 1024 * 3 * 8
    assert len(L.SIGNATURES['irs_mi_fwd']) == 19 and len(L.SIGNATURES['irs_mi_bwd']) == 19 and len(L.SIGNATURES['irs_mi_set']) == 6


def test_config_resolves_the_class():
    from ir_sgmcmc_amd.model import loss as model_loss
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_mi_l2_128.json')))
    assert cfg['data_loader']['args']['moving_contrast'] == 'invert' and cfg['virtual_decimation'] is False and cfg['trainer']['VI'] is False
    lncc = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_lncc_l2_128.json')))
    for key in ('reg_loss', 'transformation_module', 'optimizer_SG_MCMC', 'Sobolev_grad', 'trainer'):
        assert cfg[key] == lncc[key], key
    cfg['trainer']['save_dir'] = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'mi_host_config')
    config = ConfigParser.from_dict(cfg, timestamp='t')
    loss = config.init_losses()['data']['loss']
    assert isinstance(loss, model_loss.MI) and (loss.bins, loss.weight) == (cfg['data_loss']['args']['bins'], cfg['data_loss']['args']['weight'])
    assert loss.fixed_range is None and loss.moving_range is None
    with pytest.raises(NotImplementedError, match='no per-voxel map'):
        loss.map(None, None)
    with pytest.raises(NotImplementedError, match='no residual map'):
        loss.reduce(None)
    dl = config.init_data_loader()
    assert dl.moving_contrast == 'invert'


def test_engine_config_and_refusals():
    from ir_sgmcmc_amd.engine import DATA_LOSSES, EngineConfig, irs_config
    from ir_sgmcmc_amd.slab import SlabEngine
    from ir_sgmcmc_amd.trainer.trainer import mi_refusals
    assert DATA_LOSSES['MI'] == L.IRS_DATA_MI
    c = irs_config(EngineConfig(dims=(16, 16, 16), data_loss='MI', mi_bins=24, lcc_s=1, virtual_decimation=False))
    assert (c.data_loss, c.lcc_s) == (4, 24)                      # the bins travel in lcc_s
    with pytest.raises(ValueError, match='not wired'):
        irs_config(EngineConfig(dims=(16, 16, 16), data_loss='NMI'))
    with pytest.raises(L.IrsError, match='MI data term is not supported on z-slabs'):
        SlabEngine(EngineConfig(dims=(16, 16, 16), data_loss='MI', virtual_decimation=False), 'cpu', None)
    mi_refusals(False, None, False)
    with pytest.raises(ValueError, match='virtual decimation'):
        mi_refusals(True, None, False)
    with pytest.raises(ValueError, match='residual_check'):
        mi_refusals(False, {'bins': 32}, False)
    with pytest.raises(ValueError, match='VI stage'):
        mi_refusals(False, None, True)
    src = open(os.path.join(ROOT, 'ir_sgmcmc_amd', 'csrc', 'slab.hip')).read()
    assert 'cfg->data_loss == IRS_DATA_MI' in src and 'the MI data term is not supported on z-slabs' in src


def test_moving_contrast():
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    from ir_sgmcmc_amd.data_loader.data_loaders import SyntheticDataLoader
    dims = (12, 10, 14)
    f0, m0 = synthetic_pair(dims, seed=3)
    f1, m1 = synthetic_pair(dims, seed=3, moving_contrast=None)
    assert all(torch.equal(f0[k], f1[k]) and torch.equal(m0[k], m1[k]) for k in f0)       # absent: bit for bit as it always was
    fi, mi = synthetic_pair(dims, seed=3, moving_contrast='invert')
    assert torch.equal(fi['im'], f0['im']) and torch.equal(mi['mask'], m0['mask']) and torch.equal(mi['seg'], m0['seg'])
    assert torch.equal(mi['im'], m0['im'].max() + m0['im'].min() - m0['im'])
    _, mf = synthetic_pair(dims, seed=3, moving_contrast='fold')
    s = (m0['im'] - m0['im'].min()) / (m0['im'].max() - m0['im'].min())
    assert torch.equal(mf['im'], (4.0 * s * (1.0 - s)).float()) and float(mf['im'].min()) >= 0.0 and float(mf['im'].max()) <= 1.0
    with pytest.raises(ValueError, match='moving_contrast'):
        synthetic_pair(dims, moving_contrast='negate')
    fixed, moving, _ = next(iter(SyntheticDataLoader(dims, seed=3, moving_contrast='invert')))
    assert torch.equal(moving['im'][0], mi['im']) and torch.equal(fixed['im'][0], f0['im'])
    fixed, moving, _ = next(iter(SyntheticDataLoader(dims, seed=3)))
    assert torch.equal(moving['im'][0], m0['im'])
