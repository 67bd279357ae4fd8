"""Split ESS and MCSE, host side: the config option, the metric names, the ABI checks that need no device, and the estimator
restated in float64 against closed forms and against the theory of AR(1) chains."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.diagnostics import ChainMoments, diagnostics_period, ess_options
from tests._split_ess import ess_from_stats, split_ess_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = {'no_samples_MCMC': 80, 'log_period_MCMC': 10}


def _config(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['trainer'].update(trainer_over)
    return ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')


# ---------------------------------------------------------------- the config option
def test_ess_is_off_unless_asked_for():
    assert ess_options(BASE) is None
    assert ess_options({**BASE, 'convergence_diagnostics': False}) is None
    assert ess_options({**BASE, 'convergence_diagnostics': True}) is None
    assert ess_options({**BASE, 'convergence_diagnostics': {'period': 5}}) is None
    assert ess_options({**BASE, 'convergence_diagnostics': {'period': 5, 'ess': False}}) is None


def test_ess_values():
    assert ess_options({**BASE, 'convergence_diagnostics': {'period': 5, 'ess': True}}) == {'max_lag': 32, 'threshold': 400.0}
    assert ess_options({**BASE, 'convergence_diagnostics': {'ess': True}}) == {'max_lag': 32, 'threshold': 400.0}
    got = ess_options({**BASE, 'convergence_diagnostics': {'period': 1, 'ess': {'max_lag': 4, 'threshold': 100}}})
    assert got == {'max_lag': 4, 'threshold': 100.0}
    assert ess_options({**BASE, 'convergence_diagnostics': {'period': 1, 'ess': {'max_lag': 3}}})['threshold'] == 400.0
    assert ess_options({**BASE, 'convergence_diagnostics': {'period': 1, 'ess': {'threshold': 50.5}}})['max_lag'] == 32
    # the period parser accepts the new key and still gives the period
    assert diagnostics_period({**BASE, 'convergence_diagnostics': {'period': 5, 'ess': True}}) == 5
    assert diagnostics_period({**BASE, 'convergence_diagnostics': {'ess': True}}) == 10


@pytest.mark.parametrize('ess', [{'max_lag': 2}, {'max_lag': 0}, {'max_lag': -4}, {'max_lag': 4.5}, {'max_lag': '8'},
                                 {'max_lag': True}, {'threshold': 'high'}, {'threshold': None}, {'threshold': 0},
                                 {'threshold': float('nan')}, {'lag': 8}, {'max_lag': 8, 'extra': 1}, 'yes', 1, [8]])
def test_ess_refusals(ess):
    with pytest.raises(ValueError):
        ess_options({**BASE, 'convergence_diagnostics': {'period': 1, 'ess': ess}})


def test_unknown_keys_next_to_ess_are_refused():
    with pytest.raises(ValueError):
        diagnostics_period({**BASE, 'convergence_diagnostics': {'period': 1, 'ess': True, 'lags': 3}})


def test_fewer_than_four_samples_per_half_is_refused(tmp_path):
    base = {'no_samples_MCMC': 70, 'log_period_MCMC': 10}
    # 7 samples per chain: enough for R-hat (3 per half), not for ESS
    assert diagnostics_period({**base, 'convergence_diagnostics': {'period': 10, 'ess': False}}) == 10
    with pytest.raises(ValueError, match=r'no_samples_MCMC = 70 with period 10'):
        ess_options({**base, 'convergence_diagnostics': {'period': 10, 'ess': True}})
    assert ess_options({**base, 'convergence_diagnostics': {'period': 8, 'ess': True}}) is not None  # 8: 4 per half
    with pytest.raises(ValueError, match='at least 8 recorded samples'):
        ChainMoments(2, (4, 4, 4), 7, 'cpu', max_lag=4)
    # the trainer refuses the config when it is built
    from ir_sgmcmc_amd.trainer import Trainer
    config = _config(tmp_path, no_samples_MCMC=40, log_period_MCMC=10, convergence_diagnostics={'period': 6, 'ess': True})
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    with pytest.raises(ValueError, match=r'no_samples_MCMC = 40 with period 6'):
        config.init_metrics()
    with pytest.raises(ValueError, match=r'no_samples_MCMC = 40 with period 6'):
        Trainer(config, dl, losses, tm, rm, [], device='cpu')


def test_init_metrics_names_ess_after_rhat_only_when_on(tmp_path):
    rhat = ['MCMC/R_hat/max', 'MCMC/R_hat/mean', 'MCMC/R_hat/frac_above_1.01', 'MCMC/R_hat/frac_above_1.1']
    off = _config(tmp_path / 'off').init_metrics()
    on_rhat = _config(tmp_path / 'rhat', convergence_diagnostics={'period': 5}).init_metrics()
    assert on_rhat == off + rhat
    on = _config(tmp_path / 'ess', convergence_diagnostics={'period': 5, 'ess': True}).init_metrics()
    assert on == off + rhat + ['MCMC/ESS/min', 'MCMC/ESS/mean', 'MCMC/ESS/frac_below_400', 'MCMC/ESS/frac_truncated']
    thr = _config(tmp_path / 'thr', convergence_diagnostics={'period': 5, 'ess': {'threshold': 12.5}}).init_metrics()
    assert thr[-2:] == ['MCMC/ESS/frac_below_12.5', 'MCMC/ESS/frac_truncated']


# ---------------------------------------------------------------- device-free parts of the surface
def test_cpu_tensors_are_refused():
    cm = ChainMoments(2, (4, 5, 6), 8, 'cpu', max_lag=4)
    assert tuple(cm.ring.shape) == (4, 2, 3, 4, 5, 6) and tuple(cm.vsum.shape) == (4, 3, 4, 5, 6)
    with pytest.raises(L.IrsError):
        cm.record(torch.zeros(2, 3, 4, 5, 6))


def test_state_dict_carries_the_variogram_only_when_on():
    off = ChainMoments(2, (4, 5, 6), 8, 'cpu').state_dict()
    assert set(off) == {'mean', 'm2', 'count', 'n_per_chain'}
    on = ChainMoments(2, (4, 5, 6), 8, 'cpu', max_lag=5).state_dict()
    assert set(on) == {'mean', 'm2', 'count', 'n_per_chain', 'ring', 'vsum', 'max_lag'} and on['max_lag'] == 5
    on['count'] = 3
    for other in (ChainMoments(2, (4, 5, 6), 8, 'cpu', max_lag=4), ChainMoments(2, (4, 5, 6), 8, 'cpu')):
        with pytest.raises(ValueError, match='max_lag'):
            other.load_state_dict(on)
    off['count'] = 3
    with pytest.raises(ValueError, match='max_lag'):
        ChainMoments(2, (4, 5, 6), 8, 'cpu', max_lag=5).load_state_dict(off)
    same = ChainMoments(2, (4, 5, 6), 8, 'cpu', max_lag=5)
    on['vsum'] = torch.full_like(on['vsum'], 2.0)
    same.load_state_dict(on)
    assert same.count == 3 and torch.equal(same.vsum, on['vsum'])


def test_workspace_size_and_refusals():
    lib = L.load()
    n = C.c_size_t()
    assert lib.irs_split_ess_workspace(2, 7, 9, 11, C.byref(n)) == 0
    assert n.value == 5 * 8 * math.ceil(7 * 9 * 11 / 256)
    assert lib.irs_split_ess_workspace(2, 256, 256, 256, C.byref(n)) == 0 and n.value == 5 * 8 * 2048  # capped grid
    assert lib.irs_split_ess_workspace(0, 7, 9, 11, C.byref(n)) != 0
    assert lib.irs_split_ess_workspace(2, 7, 1, 11, C.byref(n)) != 0
    assert lib.irs_split_ess_workspace(2, 7, 9, 11, None) != 0
    p = C.c_void_p(16)  # never dereferenced: every call below is refused before a launch
    assert lib.irs_chain_variogram_update(p, 2, 4, 4, 4, 0, 4, p, p, None) != 0  # k < 1
    assert lib.irs_chain_variogram_update(p, 2, 4, 4, 4, 1, 0, p, p, None) != 0  # L < 1
    assert lib.irs_chain_variogram_update(p, 9, 4, 4, 4, 1, 4, p, p, None) != 0  # more chains than IRS_MAX_CHAINS
    assert lib.irs_chain_variogram_update(None, 2, 4, 4, 4, 1, 4, p, p, None) != 0
    ws = 5 * 8
    assert lib.irs_split_ess(p, p, p, 2, 3, 4, None, 400.0, p, p, p, p, ws, 4, 4, 4, None) != 0  # n - 1 < 3
    assert 'at least 4' in lib.irs_last_error().decode()
    assert lib.irs_split_ess(p, p, p, 2, 4, 0, None, 400.0, p, p, p, p, ws, 4, 4, 4, None) != 0  # L < 1
    assert lib.irs_split_ess(p, p, p, 2, 4, 4, None, 400.0, p, p, p, p, ws - 1, 4, 4, 4, None) != 0  # short workspace
    assert lib.irs_split_ess(p, p, None, 2, 4, 4, None, 400.0, p, p, p, p, ws, 4, 4, 4, None) != 0


# ---------------------------------------------------------------- the estimator against closed forms
def test_constant_field_gives_mn():
    ess, mcse, tr, _ = split_ess_np(np.full((2, 10, 3), 1.25), max_lag=8)
    assert (ess == 2 * 2 * 5).all() and (mcse == 0).all() and not tr.any()


def test_constant_within_sequences_is_truncated_with_tau_1_plus_2T():
    # every sequence constant, the sequences different: S_t = 0, rho_t = 1, no pair ever turns negative
    C, N = 2, 14
    n = N // 2
    x = np.empty((C, N))
    for c in range(C):
        x[c, :n], x[c, N - n:] = 2 * c, 2 * c + 1
        if N % 2:
            x[c, n] = 100.0
    for max_lag in (3, 4, 5, 6, 32):
        Lp = min(max_lag, n - 1)
        T = Lp if Lp % 2 else Lp - 1
        ess, mcse, tr, _ = split_ess_np(x, max_lag)
        mn = 2 * C * n
        assert tr and ess == pytest.approx(mn / (1 + 2 * T), rel=1e-14)
        vp = np.concatenate([x[:, :n], x[:, N - n:]]).mean(axis=1).var(ddof=1)
        assert mcse == pytest.approx(math.sqrt(vp / ess), rel=1e-14)


def test_short_sequences_are_refused():
    with pytest.raises(ValueError):
        split_ess_np(np.random.default_rng(0).standard_normal((2, 7)), max_lag=8)  # n = 3
    with pytest.raises(ValueError):
        ess_from_stats(np.ones(1), np.zeros((3, 1)), 4, 3, 3)


def test_antithetic_chain_hits_the_cap():
    # alternating signs: rho_1 ~ -1, tau < mn / cap, so ESS = cap = mn log10(mn)
    N = 400
    x = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[None] + 1e-3 * np.random.default_rng(1).standard_normal((1, N))
    ess, _, tr, _ = split_ess_np(x, 8)
    mn = 2 * (N // 2)
    assert ess == pytest.approx(mn * math.log10(mn), rel=1e-14) and not tr


def test_non_finite_moments_give_zero():
    x = np.random.default_rng(2).standard_normal((2, 10, 2))
    x[0, 3, 1] = np.inf
    ess, mcse, tr, _ = split_ess_np(x, 4)
    assert ess[1] == 0 and mcse[1] == np.inf and not tr[1]
    assert np.isfinite(ess[0]) and ess[0] > 0
    assert not np.isnan(ess).any() and not np.isnan(mcse).any()


# ---------------------------------------------------------------- the estimator against theory
@pytest.fixture(scope='module')
def ar1_chains():
    phi, C, N, series = 0.6, 2, 4000, 200
    rng = np.random.default_rng(2021)
    x = np.empty((C, N, series))
    x[:, 0] = rng.standard_normal((C, series)) / math.sqrt(1 - phi ** 2)
    e = rng.standard_normal((C, N, series))
    for i in range(1, N):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    return phi, x


def test_ar1_chains_match_the_theoretical_ess(ar1_chains):
    phi, x = ar1_chains
    C, N = x.shape[:2]
    mn = 2 * C * (N // 2)
    expected = mn * (1 - phi) / (1 + phi)
    ess, mcse, tr, _ = split_ess_np(x, max_lag=32)
    assert abs(ess.mean() / expected - 1) < 0.1, (ess.mean(), expected)
    # MCSE of the mean: sqrt(var / ESS), var = 1 / (1 - phi^2)
    assert abs(np.median(mcse) / math.sqrt(1 / (1 - phi ** 2) / expected) - 1) < 0.1
    # rho_t = 0.6^t is below the estimate's noise (about 0.01) from lag 9 on, and a few series' noisy tails keep every pair
    # rho_{T+1} + rho_{T+2} up to lag 32 positive: those are flagged as truncated
    assert tr.mean() < 0.1
    # a longer window finds a negative pair for every series and hardly moves the estimate
    ess64, _, tr64, _ = split_ess_np(x, max_lag=64)
    assert not tr64.any()
    assert abs(ess64.mean() / ess.mean() - 1) < 0.01
