"""Displacement credible intervals, the part that needs no GPU: the option parser and every refusal, the summary arithmetic, the
numpy restatement on a hand-checked case, and the properties the GPU test then holds the device to, checked here on the very
same inputs: the restated quantile lies within one bin width of the order statistic x_(ceil(p n)), is non-decreasing in p, and
the in-range cases really are in range."""
import math

import numpy as np
import pytest

from ir_sgmcmc_amd.diagnostics import (QUANTILE_METRICS, QUANTILE_OPTION_KEYS, DisplacementQuantiles,
                                       displacement_quantiles_options, quantiles_summary)
from ir_sgmcmc_amd.logger import quantile_tag
from tests._displacement_quantiles import (BIN_WIDTH, CASES, CLIP_CASE, CLIP_NOISE, HAND_BIN_WIDTH, HAND_CI, HAND_OFFSETS,
                                           HAND_PROBS, HAND_SCALE, IN_RANGE_CASES, PROBS, bins_np, case_mask, case_seed,
                                           check_bound, check_monotone, default_scale, draw_records, finalize_np,
                                           hand_checked_records, histogram_np, quantiles_np, summary_np, widths)

BASE = {'log_period_MCMC': 5, 'no_samples_MCMC': 100, 'no_chains': 2}


def test_option_off_and_defaults():
    assert QUANTILE_OPTION_KEYS == ('period', 'probs', 'bins', 'bin_width')
    assert QUANTILE_METRICS == ('width_mean', 'width_max', 'width_x', 'width_y', 'width_z', 'out_of_range_frac', 'clipped_frac')
    for off in ({}, {'displacement_quantiles': False}, {'displacement_quantiles': None}):
        assert displacement_quantiles_options({**BASE, **off}) is None
    want = {'period': 5, 'probs': (0.05, 0.5, 0.95), 'bins': 64, 'bin_width': 0.125}
    assert displacement_quantiles_options({**BASE, 'displacement_quantiles': True}) == want
    assert displacement_quantiles_options({**BASE, 'displacement_quantiles': {}}) == want
    got = displacement_quantiles_options({**BASE, 'displacement_quantiles': {'period': 2, 'probs': [0.025, 0.975], 'bins': 128,
                                                                             'bin_width': 0.25}})
    assert got == {'period': 2, 'probs': (0.025, 0.975), 'bins': 128, 'bin_width': 0.25}
    assert displacement_quantiles_options({**BASE, 'displacement_quantiles': {'bin_width': 1}})['bin_width'] == 1.0


@pytest.mark.parametrize('opt,match', [
    ({'perod': 2}, 'unknown keys'),
    ('yes', 'must be true'),
    (3, 'must be true'),
    ({'period': 2.0}, 'integer'),
    ({'period': True}, 'integer'),
    ({'period': 0}, '>= 1'),
    ({'period': 101}, 'records no step'),
    ({'probs': 0.5}, 'list'),
    ({'probs': '0.5'}, 'list'),
    ({'probs': [0.5]}, '2 to 8'),
    ({'probs': [0.1 * k for k in range(1, 10)]}, '2 to 8'),
    ({'probs': [0.5, 0.5]}, 'increasing'),
    ({'probs': [0.9, 0.1]}, 'increasing'),
    ({'probs': [0.0, 0.5]}, 'increasing'),
    ({'probs': [0.5, 1.0]}, 'increasing'),
    ({'probs': [0.5, float('nan')]}, 'increasing'),
    ({'probs': [0.1, '0.5']}, 'numbers'),
    ({'probs': [True, 0.5]}, 'numbers'),
    ({'bins': 63}, 'even'),
    ({'bins': 2}, 'even'),
    ({'bins': 258}, 'even'),
    ({'bins': 64.0}, 'integer'),
    ({'bins': True}, 'integer'),
    ({'bin_width': 0}, 'bin_width'),
    ({'bin_width': -0.1}, 'bin_width'),
    ({'bin_width': float('inf')}, 'bin_width'),
    ({'bin_width': float('nan')}, 'bin_width'),
    ({'bin_width': '0.1'}, 'bin_width'),
    ({'bin_width': True}, 'bin_width'),
])
def test_option_refusals(opt, match):
    with pytest.raises(ValueError, match=match):
        displacement_quantiles_options({**BASE, 'displacement_quantiles': opt})


def test_more_records_than_a_count_holds_are_refused_and_the_message_names_the_period():
    cfg = {'log_period_MCMC': 1, 'no_samples_MCMC': 65535, 'no_chains': 1, 'displacement_quantiles': True}
    assert displacement_quantiles_options(cfg)['period'] == 1  # 65535 records: the most a uint16 count holds
    with pytest.raises(ValueError, match='raise `period`'):
        displacement_quantiles_options({**cfg, 'no_samples_MCMC': 65536})
    with pytest.raises(ValueError, match='raise `period`'):
        displacement_quantiles_options({**cfg, 'no_chains': 2, 'no_samples_MCMC': 40000})
    assert displacement_quantiles_options({**cfg, 'no_chains': 2, 'no_samples_MCMC': 40000,
                                           'displacement_quantiles': {'period': 2}})['period'] == 2


def test_quantile_tag():
    assert [quantile_tag(p) for p in (0.05, 0.5, 0.95, 0.025, 0.975, 0.001)] == ['5', '50', '95', '2p5', '97p5', '0p1']


def test_quantiles_summary():
    s = quantiles_summary([10, 2, 6], [4.0, 0.9, 1.6, 2.4, 0.8], 5)
    assert (s['records'], s['voxels'], s['out_of_range_voxels'], s['clipped_samples']) == (5, 10, 2, 6)
    assert s['width_mean'] == 0.5 and s['width_max'] == 0.9 and (s['width_x'], s['width_y'], s['width_z']) == (0.2, 0.3, 0.1)
    assert s['out_of_range_frac'] == 0.2 and s['clipped_frac'] == 6 / 150
    assert set(QUANTILE_METRICS) <= set(s)
    empty = quantiles_summary([0, 0, 0], [0.0, -math.inf, 0.0, 0.0, 0.0], 5)
    assert empty['voxels'] == 0 and all(math.isnan(empty[k]) for k in QUANTILE_METRICS)
    none_inside = quantiles_summary([3, 3, 40], [0.0, -math.inf, 0.0, 0.0, 0.0], 5)
    assert none_inside['out_of_range_frac'] == 1.0 and none_inside['clipped_frac'] == 40 / 45
    assert all(math.isnan(none_inside[k]) for k in ('width_mean', 'width_max', 'width_x', 'width_y', 'width_z'))


def test_the_class_refuses_bad_arguments_before_it_touches_a_device():
    for kw in (dict(dims=(4, 4)), dict(dims=(1, 4, 4)), dict(bins=5), dict(bins=2), dict(bins=512), dict(bin_width=0.0),
               dict(bin_width=float('nan')), dict(scale=(1.0, 1.0)), dict(scale=(1.0, 0.0, 1.0)), dict(scale=(1.0, float('inf'), 1.0)),
               dict(bin_width=1e-45, scale=(1e30, 1.0, 1.0))):
        args = {'dims': (4, 5, 6), **kw}
        with pytest.raises(ValueError):
            DisplacementQuantiles(args.pop('dims'), 'cpu', **args)
    assert DisplacementQuantiles.bytes_per_voxel(64) == 396
    assert DisplacementQuantiles.bytes_per_voxel(64) * 256 ** 3 == pytest.approx(6.6e9, rel=0.01)


def test_bins_of_the_restatement():
    B = 8
    iw = np.full(3, 2.0, dtype=np.float32)  # width 0.5
    c = np.zeros((3, 1), dtype=np.float32)
    x = lambda v: np.full((3, 1), v, dtype=np.float32)
    for v, want in ((0.0, 4), (0.49, 4), (0.5, 5), (-0.01, 3), (-0.5, 3), (-0.51, 2), (1.49, 6), (1.5, 7), (100.0, 7), (-1.5, 1),
                    (-1.51, 0), (-100.0, 0), (np.inf, 7), (-np.inf, 0), (np.nan, 0), (3e38, 7)):
        assert (bins_np(x(v), c, iw, B) == want).all(), v
    assert (bins_np(x(1.0), x(np.nan), iw, B) == 0).all() and (bins_np(x(np.inf), x(np.inf), iw, B) == 0).all()


def test_hand_checked_case():
    records, centre = hand_checked_records()
    ref = quantiles_np(records, HAND_PROBS, bins=8, bin_width=HAND_BIN_WIDTH, scale=HAND_SCALE)
    assert ref['width'].tolist() == [0.5] * 3 and ref['inv_width'].tolist() == [2.0] * 3
    assert np.array_equal(ref['centre'], centre.astype(np.float32))
    assert (ref['hist'][:, 4] == 2).all() and (ref['hist'][:, 5] == 2).all() and ref['hist'].sum() == 4 * centre.size
    for j, off in enumerate(HAND_OFFSETS):
        assert np.array_equal(ref['quantiles'][j], (2.0 * (centre + off)).astype(np.float32))
    assert np.array_equal(ref['ci_width'], np.full(centre.shape[1:], HAND_CI, dtype=np.float32))
    s = ref['summary']
    assert (s['voxels'], s['out_of_range_voxels'], s['clipped_samples']) == (60, 0, 0)
    assert s['width_mean'] == pytest.approx(HAND_CI, rel=1e-7) and s['width_x'] == s['width_y'] == s['width_z'] == 1.0
    check_bound(records, HAND_PROBS, ref['quantiles'], HAND_BIN_WIDTH, HAND_SCALE)
    # two bins only hold the records: with 4 bins the upper one is the open-ended bin 3 and the 0.75 quantile is out of range
    ref4 = quantiles_np(records, HAND_PROBS, bins=4, bin_width=HAND_BIN_WIDTH, scale=HAND_SCALE)
    assert np.isnan(ref4['quantiles'][2]).all() and np.isfinite(ref4['quantiles'][:2]).all() and np.isnan(ref4['ci_width']).all()
    assert ref4['summary']['out_of_range_frac'] == 1.0 and ref4['summary']['clipped_samples'] == 2 * centre.size
    assert math.isnan(ref4['summary']['width_mean'])


@pytest.mark.parametrize('C,steps,shape,bins', IN_RANGE_CASES)
def test_in_range_cases_are_in_range_and_within_a_bin_of_the_order_statistic(C, steps, shape, bins):
    n = C * steps
    records = draw_records(n, shape, case_seed(C, steps, shape, bins))
    ref = quantiles_np(records, PROBS, bins=bins, bin_width=BIN_WIDTH)
    assert (ref['hist'].sum(axis=1) == n).all()
    assert ref['summary']['out_of_range_voxels'] == 0 and np.isfinite(ref['quantiles']).all() and np.isfinite(ref['ci_width']).all()
    check_bound(records, PROBS, ref['quantiles'], BIN_WIDTH, ref['scale'])
    check_monotone(ref['quantiles'])
    more = (0.01, 0.05, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99)
    q8, _ = finalize_np(ref['centre'], ref['hist'], n, ref['width'], ref['scale'], more)
    check_monotone(q8)
    check_bound(records, more, q8, BIN_WIDTH, ref['scale'], where=np.isfinite(q8).all(axis=0))


def test_the_clipping_case_clips():
    C, steps, shape, bins = CLIP_CASE
    n = C * steps
    records = draw_records(n, shape, case_seed(*CLIP_CASE), noise=CLIP_NOISE)
    mask = case_mask(shape)
    ref = quantiles_np(records, PROBS, bins=bins, bin_width=BIN_WIDTH, mask=mask)
    s = ref['summary']
    V = int(np.prod(shape))
    bad = np.isnan(ref['quantiles']).any(axis=(0, 1))
    print({'out of range': int(bad.sum()), 'of': V, 'clipped_frac': s['clipped_frac']})
    assert 0.25 * V < bad.sum() < 0.95 * V and s['out_of_range_voxels'] == int((bad & mask).sum()) and s['clipped_samples'] > 0
    assert 0 < s['out_of_range_voxels'] < s['voxels'] and math.isfinite(s['width_mean'])
    assert np.array_equal(np.isnan(ref['ci_width']), bad)
    check_monotone(ref['quantiles'])
    for j in range(len(PROBS)):  # the quantiles that are in range still hold the bound, voxel and channel by channel
        ok = np.isfinite(ref['quantiles'][j])
        check_bound(records, PROBS[j:j + 1], ref['quantiles'][j:j + 1], BIN_WIDTH, ref['scale'], where=ok)


@pytest.mark.parametrize('C,steps,shape,bins', CASES)
def test_counts_commute_and_every_voxel_holds_n(C, steps, shape, bins):
    n = C * steps
    records = draw_records(n, shape, case_seed(C, steps, shape, bins))
    _, iw = widths(BIN_WIDTH, default_scale(shape))
    centre, hist = histogram_np(records, bins, iw)
    assert (hist.sum(axis=1) == n).all() and np.array_equal(centre, records[0])
    order = np.concatenate([[0], np.random.default_rng(1).permutation(np.arange(1, n))]).astype(int)
    _, again = histogram_np(records[order], bins, iw)
    assert np.array_equal(hist, again)
    w, _ = widths(BIN_WIDTH, default_scale(shape))
    q, ci = finalize_np(centre, hist, n, w, default_scale(shape), PROBS)
    check_monotone(q)
    s = summary_np(n, hist, q, ci, case_mask(shape))
    assert s['voxels'] == int(case_mask(shape).sum()) and 0 <= s['clipped_frac'] <= 1
