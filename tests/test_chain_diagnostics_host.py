"""Split-R-hat convergence diagnostics, host side: the recording schedule, the config option, the metric names, the ABI
checks that need no device, and the estimator itself restated in float64 on sequences with a known R-hat."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.diagnostics import ChainMoments, diagnostics_period, is_recorded, recorded_steps
from tests._split_rhat import split_rhat_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(tmp_path, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['trainer'].update(trainer_over)
    return ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')


# ---------------------------------------------------------------- schedule
def test_schedule_even():
    assert ChainMoments.schedule(6) == [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3)]


def test_schedule_odd_skips_the_middle_sample():
    assert ChainMoments.schedule(5) == [(0, 1), (0, 2), None, (1, 1), (1, 2)]
    assert ChainMoments.schedule(9).count(None) == 1 and ChainMoments.schedule(9)[4] is None


def test_schedule_minimal():
    assert ChainMoments.schedule(4) == [(0, 1), (0, 2), (1, 1), (1, 2)]


@pytest.mark.parametrize('N', range(4, 40))
def test_schedule_halves_are_equal_and_ordered(N):
    s = ChainMoments.schedule(N)
    for h in (0, 1):
        ks = [slot[1] for slot in s if slot is not None and slot[0] == h]
        assert ks == list(range(1, N // 2 + 1))
    first1 = next(i for i, slot in enumerate(s) if slot is not None and slot[0] == 1)
    assert first1 == N - N // 2


# ---------------------------------------------------------------- which transitions are recorded
@pytest.mark.parametrize('burn_in,samples,period,expected', [
    (4, 10, 2, [6, 8, 10, 12, 14]),
    (0, 8, 2, [2, 4, 6, 8]),
    (5, 13, 3, [8, 11, 14, 17]),
    (20, 40, 10, [30, 40, 50, 60]),
    (3, 7, 1, [4, 5, 6, 7, 8, 9, 10]),
])
def test_recorded_steps(burn_in, samples, period, expected):
    got = recorded_steps(burn_in, samples, period)
    assert got == expected and len(got) == samples // period
    # the predicate the trainer's loop applies, over the whole run (burn-in included)
    assert [s for s in range(1, burn_in + samples + 1) if is_recorded(s, burn_in, period)] == expected


# ---------------------------------------------------------------- the config option
def test_option_values():
    base = {'no_samples_MCMC': 40, 'log_period_MCMC': 10}
    assert diagnostics_period(base) is None
    assert diagnostics_period({**base, 'convergence_diagnostics': False}) is None
    assert diagnostics_period({**base, 'convergence_diagnostics': True}) == 10
    assert diagnostics_period({**base, 'convergence_diagnostics': {'period': 5}}) == 5
    with pytest.raises(ValueError):
        diagnostics_period({**base, 'convergence_diagnostics': 'yes'})
    with pytest.raises(ValueError):
        diagnostics_period({**base, 'convergence_diagnostics': {'period': 0}})


def test_fewer_than_two_samples_per_half_is_refused(tmp_path):
    base = {'no_samples_MCMC': 30, 'log_period_MCMC': 10}
    with pytest.raises(ValueError, match=r'no_samples_MCMC = 30 with period 10'):
        diagnostics_period({**base, 'convergence_diagnostics': True})
    assert diagnostics_period({**base, 'convergence_diagnostics': {'period': 7}}) == 7  # 4 samples: 2 per half
    with pytest.raises(ValueError, match='at least 4 recorded samples'):
        ChainMoments(2, (4, 4, 4), 3, 'cpu')
    # the trainer refuses the config when it is built
    from ir_sgmcmc_amd.trainer import Trainer
    config = _config(tmp_path, no_samples_MCMC=40, log_period_MCMC=10, convergence_diagnostics={'period': 11})
    dl = config.init_data_loader()
    losses = config.init_losses()
    tm, rm = config.init_transformation_and_registration_modules()
    with pytest.raises(ValueError, match=r'no_samples_MCMC = 40 with period 11'):
        Trainer(config, dl, losses, tm, rm, config.init_metrics(), device='cpu')


def test_init_metrics_names_rhat_only_when_on(tmp_path):
    keys = ['MCMC/R_hat/max', 'MCMC/R_hat/mean', 'MCMC/R_hat/frac_above_1.01', 'MCMC/R_hat/frac_above_1.1']
    off = _config(tmp_path / 'off').init_metrics()
    assert not [m for m in off if 'R_hat' in m]
    assert off == _config(tmp_path / 'false', convergence_diagnostics=False).init_metrics()
    on = _config(tmp_path / 'on', convergence_diagnostics=True).init_metrics()
    assert on[:len(off)] == off and on[len(off):] == keys


# ---------------------------------------------------------------- device-free parts of the surface
def test_cpu_tensors_are_refused():
    cm = ChainMoments(2, (4, 5, 6), 4, 'cpu')
    with pytest.raises(L.IrsError):
        cm.record(torch.zeros(2, 3, 4, 5, 6))


def test_workspace_size_and_refusals():
    lib = L.load()
    n = C.c_size_t()
    assert lib.irs_split_rhat_workspace(2, 7, 9, 11, C.byref(n)) == 0
    assert n.value == 5 * 8 * math.ceil(7 * 9 * 11 / 256)
    assert lib.irs_split_rhat_workspace(2, 256, 256, 256, C.byref(n)) == 0 and n.value == 5 * 8 * 2048  # capped grid
    assert lib.irs_split_rhat_workspace(0, 7, 9, 11, C.byref(n)) != 0
    assert lib.irs_split_rhat_workspace(2, 0, 9, 11, C.byref(n)) != 0
    assert lib.irs_split_rhat_workspace(2, 7, 9, 11, None) != 0


# ---------------------------------------------------------------- the estimator on sequences with a known R-hat
def _chains(base, shifts):
    """chain c = [base + shifts[c][0], (middle), base + shifts[c][1]]: every sequence is `base` shifted"""
    return np.array([np.concatenate([base + s0, base + s1]) for s0, s1 in shifts])


def test_equal_constant_chains_give_one():
    assert split_rhat_np(np.full((2, 6), 3.5)) == 1.0
    assert split_rhat_np(np.full((3, 7), -1.0)) == 1.0


def test_identical_sequences_give_the_within_only_value():
    base = np.array([0.0, 1.0, 3.0, 2.0])
    n = len(base)
    r = split_rhat_np(_chains(base, [(0, 0), (0, 0)]))
    assert r == pytest.approx(math.sqrt((n - 1) / n), rel=1e-15)


@pytest.mark.parametrize('shifts', [[(0, 0), (1, 1)], [(0, 2), (0, 2)], [(0.5, -1), (2, 0), (3, 1)], [(0, 10)]])
def test_shifted_sequences_give_the_closed_form(shifts):
    base = np.array([1.0, -2.0, 0.5, 4.0, 3.0])
    n = len(base)
    s2 = base.var(ddof=1)
    flat = np.array(shifts, dtype=np.float64).reshape(-1)
    expected = math.sqrt(((n - 1) / n * s2 + flat.var(ddof=1)) / s2)
    assert split_rhat_np(_chains(base, shifts)) == pytest.approx(expected, rel=1e-14)


def test_the_middle_sample_of_an_odd_count_is_ignored():
    base = np.array([1.0, 2.0, 4.0])
    even = _chains(base, [(0, 1), (1, 0)])
    odd = np.array([np.concatenate([c[:3], [1e6], c[3:]]) for c in even])
    assert split_rhat_np(odd) == split_rhat_np(even)


def test_zero_within_variance():
    assert split_rhat_np(np.array([[2.0] * 4, [3.0] * 4])) == math.inf              # W = 0 < B
    assert split_rhat_np(np.array([[2.0, 2.0, 3.0, 3.0]])) == math.inf              # one chain, halves differ
    assert split_rhat_np(np.array([[2.0, 2.0, 9.0, 2.0, 2.0]])) == 1.0             # W = B = 0 (middle ignored)
    assert not np.isnan(split_rhat_np(np.zeros((2, 4, 3)))).any()
