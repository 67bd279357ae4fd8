"""Host side of the inverse-consistency feature: the `trainer.inverse_consistency` option, the proof that the exact cases of
the GPU test are exact (the fp32 and the fp64 evaluation of tests/_inverse_consistency.py agree bit for bit, as
tests/test_exact_cases_host.py proves for the warp family), and the helper's Welford / peak update against torch.mean /
torch.amax."""
import math

import pytest
import torch

from ir_sgmcmc_amd.diagnostics import (ICE_DEFAULTS, ice_chain_summary, ice_map_summary, inverse_consistency_options,
                                       recorded_steps)
from tests import _exact_cases as X
from tests import _inverse_consistency as R


def cfg(**over):
    return {'no_samples_MCMC': 8, 'log_period_MCMC': 4, 'no_chains': 2, **over}


def test_options_off_and_defaults():
    for off in ({}, {'inverse_consistency': False}, {'inverse_consistency': None}):
        assert inverse_consistency_options(cfg(**off)) is None
    assert inverse_consistency_options(cfg(inverse_consistency=True)) == {'period': 4, **ICE_DEFAULTS}
    assert ICE_DEFAULTS == {'threshold': 0.5, 'moving_space_dice': False}
    got = inverse_consistency_options(cfg(inverse_consistency={'period': 2, 'threshold': 1, 'moving_space_dice': True}))
    assert got == {'period': 2, 'threshold': 1.0, 'moving_space_dice': True} and isinstance(got['threshold'], float)
    assert inverse_consistency_options(cfg(inverse_consistency={}))['period'] == 4
    assert len(recorded_steps(3, 8, got['period'])) == 4


@pytest.mark.parametrize('opt, message', [
    ({'periodd': 2}, r"trainer\.inverse_consistency: unknown keys \['periodd'\]; known: \['period', 'threshold', 'moving_space_dice'\]"),
    ({'threshold': float('nan')}, r'trainer\.inverse_consistency\.threshold must be a finite number > 0 \(voxels\), got nan'),
    ({'threshold': float('inf')}, r'trainer\.inverse_consistency\.threshold must be a finite number > 0 \(voxels\), got inf'),
    ({'threshold': 0}, r'trainer\.inverse_consistency\.threshold must be a finite number > 0 \(voxels\), got 0'),
    ({'threshold': -0.5}, r'trainer\.inverse_consistency\.threshold must be a finite number > 0 \(voxels\), got -0\.5'),
    ({'threshold': '0.5'}, r"trainer\.inverse_consistency\.threshold must be a finite number > 0 \(voxels\), got '0\.5'"),
    ({'threshold': True}, r'trainer\.inverse_consistency\.threshold must be a finite number > 0 \(voxels\), got True'),
    ({'moving_space_dice': 1}, r'trainer\.inverse_consistency\.moving_space_dice must be true or false, got 1'),
    ({'period': 9}, r'trainer\.inverse_consistency: no_samples_MCMC = 8 with period 9 records no step'),
    ({'period': 0}, r'trainer\.inverse_consistency: the period must be >= 1, got 0'),
    ({'period': 2.0}, r'trainer\.inverse_consistency\.period must be an integer, got 2\.0'),
    ('yes', r'trainer\.inverse_consistency must be true, false or \{"period": P, "threshold": t, "moving_space_dice": bool\}, got \'yes\''),
])
def test_options_refusals(opt, message):
    with pytest.raises(ValueError, match=message):
        inverse_consistency_options(cfg(inverse_consistency=opt))


def test_summaries_from_columns():
    s = ice_chain_summary([10, 2], [4.0, 8.0, 1.5])
    assert s == {'voxels': 10, 'nonfinite_voxels': 2, 'mean': 0.5, 'rms': 1.0, 'max': 1.5}
    e = ice_chain_summary([3, 3], [0.0, 0.0, float('-inf')])
    assert math.isnan(e['mean']) and math.isnan(e['rms']) and math.isnan(e['max'])
    m = ice_map_summary([8, 0, 2], [2.0, 0.75, 1.25], 6, 0.5)
    assert m == {'records': 6, 'voxels': 8, 'nonfinite_voxels': 0, 'mean': 0.25, 'mean_max': 0.75, 'max': 1.25, 'above_0.5': 2,
                 'frac_above_0.5': 0.25}
    z = ice_map_summary([0, 0, 0], [0.0, float('-inf'), float('-inf')], 6, 0.5)
    assert all(math.isnan(z[k]) for k in ('mean', 'mean_max', 'max', 'frac_above_0.5'))


@pytest.mark.parametrize('dims', X.EXACT_DIMS)
def test_exact_cases_are_exact(dims):
    """on every case the GPU test holds to torch.equal, the composition evaluated in fp32 is the one evaluated in fp64"""
    t_a, d_a, d_b = R.exact_case(dims)
    assert t_a.shape == d_a.shape == d_b.shape == (X.CHAINS, 3, *dims)
    r32, _ = R.compose(t_a, d_a, d_b, torch.float32)
    r64, _ = R.compose(t_a, d_a, d_b, torch.float64)
    assert r32.dtype == torch.float32 and r64.dtype == torch.float64
    assert torch.equal(r32.double(), r64) and torch.equal(r64.float().double(), r64)
    assert float(r64.abs().max()) > 1.0  # not a trivial field
    # the positions reach past every face and sit on the borders: the clamp is exercised on every axis
    for raw, n in zip(X.voxel_coordinates(t_a, dims), X.axis_sizes(dims)):
        assert float(raw.min()) == -3.0 and float(raw.max()) == n - 1 + 3.0
        assert bool((raw == 0).any()) and bool((raw == n - 1).any())
    # the helper's sampler is the oracle's explicit restatement of it
    ex = O_explicit(t_a, d_b)
    assert torch.equal(ex + d_a.double(), r64)


def O_explicit(t_a, d_b):
    from oracle import ops as O
    return O.trilinear_sample_explicit(d_b.double(), t_a.double().permute(0, 2, 3, 4, 1))


def test_welford_and_peak_update_match_mean_and_amax():
    g = torch.Generator().manual_seed(0)
    dims, C, steps = (3, 4, 5), 2, 3
    recs = torch.rand(steps, C, 1, *dims, generator=g, dtype=torch.float64) * 3.0
    recs[1, 0, 0, 1, 2, 3] = float('nan')   # one NaN record at one voxel
    recs[:, :, 0, 0, 0, 0] = float('nan')   # a voxel no record is finite at
    recs[2, 1, 0, 2, 1, 1] = float('inf')   # non-finite, but no NaN
    state = (torch.full(dims, 7.0, dtype=torch.float64),) * 2   # stale state: records_before = 0 must ignore it
    for i in range(steps):
        state = R.update(state, recs[i], i * C, torch.float64)
    mean, peak = state
    stacked = recs.reshape(steps * C, *dims)
    want_mean = stacked.mean(dim=0)
    finite = torch.isfinite(want_mean)
    assert torch.equal(torch.isnan(mean), torch.isnan(want_mean)) and bool(torch.isnan(mean[1, 2, 3])) and bool(torch.isnan(mean[0, 0, 0]))
    assert float(mean[2, 1, 1]) == float('inf')
    assert float((mean[finite] - want_mean[finite]).abs().max()) <= 8 * 2.0 ** -52 * 3.0
    want_peak = torch.where(torch.isfinite(stacked), stacked, torch.full_like(stacked, float('-inf'))).amax(dim=0)
    none = torch.isinf(want_peak)
    assert int(none.sum()) == 1 and bool(none[0, 0, 0]) and torch.equal(torch.isnan(peak), none)
    assert torch.equal(peak[~none], want_peak[~none])
    # the same in fp32 on fp32 records: the peak is a selection and stays exact
    state32 = None
    for i in range(steps):
        state32 = R.update(state32, recs[i].float(), i * C, torch.float32)
    assert state32[0].dtype == torch.float32
    want32 = torch.where(torch.isfinite(stacked), stacked, torch.full_like(stacked, float('-inf'))).float().amax(dim=0)
    assert torch.equal(state32[1][~none], want32[~none])
    # the summary columns of the two maps
    ints, floats = R.map_summary(mean, peak, 2.5)
    assert ints == [60, int((~torch.isfinite(mean)).sum()), int((peak[~none] > 2.5).sum())]
    assert floats[2] == float(want_peak[~none].max())
