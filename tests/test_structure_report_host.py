"""Structure report on the host: the restatement on a hand-checked case, the summary maths (coherence of a block and of
independent voxels, the shared split R-hat), option parsing and every refusal, the metric names, and the CSV round trip.  No GPU:
the reductions themselves are tests/test_gpu_structure_report.py's."""
import math

import numpy as np
import pytest

from ir_sgmcmc_amd import structure_report as sr
from ir_sgmcmc_amd.diagnostics import displacement_covariance_options  # noqa: F401  (the option the coherence keys depend on)
from ir_sgmcmc_amd.modes import split_rhat_series
from ir_sgmcmc_amd.parse_config import ConfigParser
from tests._structure_report import (covariance_trace_np, identity_np, label_values, label_volume, map_stats_np, motion_np,
                                     split_rhat_np, structure_index_np, summary_np)

BASE = {'no_samples_MCMC': 12, 'log_period_MCMC': 4, 'no_chains': 2, 'no_iters_burn_in': 3}


def hand_case():
    """(5,9,17): 2 / (N - 1) is dyadic, so the identity and x * 1.25 are exact in float32 and det = 1.25 at every voxel.
    Structure 7 is the z < 2 slab (2 * 9 * 17 = 306 voxels), structure 3 the z == 4 plane (153); plane z == 2 holds label 0,
    plane z == 3 the unlisted label 99.  Constant dyadic displacements per structure whose scaled norms are
    integers (3 and 7), scale (0.5, 1, 2): every sum is exact in any order."""
    shape = (5, 9, 17)
    seg = np.zeros(shape, dtype=np.int16)
    seg[:2], seg[3], seg[4] = 7, 99, 3
    t = identity_np(shape)[None].copy()
    t[:, 0] *= 1.25
    u = np.zeros((1, 3) + shape, dtype=np.float32)
    u[0, :, :2] = np.array([2.0, -2.0, 1.0], dtype=np.float32).reshape(3, 1, 1, 1)
    u[0, :, 4] = np.array([-4.0, 3.0, 3.0], dtype=np.float32).reshape(3, 1, 1)
    u[0, :, 2:4] = 1000.0  # belongs to no structure: must not be seen
    return shape, seg, t.astype(np.float32), u, (7, 3), (0.5, 1.0, 2.0)


# per structure: w = u * scale, |w|^2, |w|
HAND = {7: ((1.0, -2.0, 2.0), 9.0, 3.0, 306), 3: ((-2.0, 3.0, 6.0), 49.0, 7.0, 153)}


def test_hand_checked_case():
    shape, seg, t, u, labels, scale = hand_case()
    out = motion_np(u, t, seg, labels, scale)
    for j, lab in enumerate(labels):
        w, n2, n1, vox = HAND[lab]
        assert out['ints'][0, j].tolist() == [vox, 0]
        f = out['floats'][0, j]
        assert f[0:3].tolist() == [vox * w[0], vox * w[1], vox * w[2]]
        assert f[3] == vox * n1 and f[4] == vox * n2 and f[5] == n1
        assert f[6] == 1.25 * vox and f[7] == 1.25 and f[8] == 1.25
    table = sr.structure_summary(out['ints'], out['floats'], ['a', 'b'], spacing=(2.0, 1.0, 0.5))
    assert table['records'] == 1
    a = table['structures']['a']
    assert (a['voxels'], a['shift_mean_x'], a['shift_mean_y'], a['shift_mean_z']) == (306, 1.0, -2.0, 2.0)
    assert a['shift_mean_norm'] == 3.0 and a['disp_rms'] == 3.0 and a['disp_mean'] == 3.0
    assert a['vol_ratio_mean'] == 1.25 and a['vol_mean_mm3'] == 1.25 * 306 and a['fold_frac'] == 0.0
    assert (a['det_min'], a['det_max'], a['disp_max']) == (1.25, 1.25, 3.0)
    assert all(math.isnan(a[k]) for k in ('shift_std_major', 'shift_std_minor', 'shift_std_total', 'vol_ratio_std', 'rhat_max'))
    assert 'coherence' not in a and list(a) == list(sr.MOTION_KEYS)


def test_membership_mask_and_empty_structures():
    shape = (4, 5, 6)
    labels = label_values(3) + [4242]  # the last one appears nowhere
    seg = label_volume('white', shape, labels[:3], 1)
    mask = np.random.default_rng(0).random(shape) < 0.5
    idx = structure_index_np(seg, labels, mask)
    assert set(np.unique(idx)) == {-1, 0, 1, 2} and (idx[~mask.reshape(-1)] == -1).all()
    assert (idx[(seg.reshape(-1) == 0) | (seg.reshape(-1) == -3) | (seg.reshape(-1) == 9999)] == -1).all()
    rng = np.random.default_rng(1)
    u = rng.normal(size=(2, 3) + shape).astype(np.float32)
    t = identity_np(shape)[None].repeat(2, axis=0)
    out = motion_np(u, t, seg, labels, mask=mask)
    assert out['ints'][:, 3].tolist() == [[0, 0], [0, 0]]
    assert out['floats'][0, 3].tolist() == [0, 0, 0, 0, 0, -math.inf, 0, math.inf, -math.inf]
    row = sr.structure_summary(out['ints'], out['floats'], list('abcd'), chains=2)['structures']['d']
    assert row['voxels'] == 0 and all(math.isnan(row[k]) for k in sr.MOTION_KEYS[1:])
    maps = rng.normal(size=(2,) + shape).astype(np.float32)
    maps[0, 0, 0, :3] = (np.nan, np.inf, -np.inf)
    ms = map_stats_np(maps, seg, labels)
    assert ms['ints'][:, 3].tolist() == [[0, 0], [0, 0]] and ms['floats'][0, 3].tolist() == [0, 0, math.inf, -math.inf]
    assert ms['ints'][0].sum() == (structure_index_np(seg, labels) >= 0).sum()
    rows = sr.structure_map_rows(ms['ints'], ms['floats'], ['m0', 'm1'], list('abcd'))
    assert rows['d']['m0_finite'] == 0 and math.isnan(rows['d']['m0_mean']) and math.isnan(rows['d']['m1_max'])
    g = structure_index_np(seg, labels) == 1
    x = maps[1].reshape(-1)[g].astype(np.float64)
    assert rows['b']['m1_mean'] == pytest.approx(x.mean(), rel=1e-12) and rows['b']['m1_std'] == pytest.approx(x.std(), rel=1e-9)
    assert (rows['b']['m1_min'], rows['b']['m1_max'], rows['b']['m1_finite']) == (x.min(), x.max(), x.size)


def series_of(records, seg, labels, scale=(1.0, 1.0, 1.0)):
    """records (n,3,D,H,W) displacements under the identity transformation -> (ints (n,K,2), floats (n,K,9))"""
    t = identity_np(records.shape[2:])[None].repeat(records.shape[0], axis=0)
    out = motion_np(records, t, seg, labels, scale)
    return out['ints'], out['floats']


def test_coherence_of_a_block_and_of_independent_voxels():
    shape, labels = (6, 7, 8), [5, 6]
    seg = np.full(shape, 5, dtype=np.int16)
    seg[3:] = 6
    rng = np.random.default_rng(3)
    n, scale = 12, (0.5, 1.0, 2.0)
    # every voxel of a structure moves by the same dyadic vector in a record: the structure moves as one block
    block = np.zeros((n, 3) + shape, dtype=np.float32)
    for r in range(n):
        block[r, :, :3] = (rng.integers(-64, 64, size=3) / 16.0).astype(np.float32).reshape(3, 1, 1, 1)
        block[r, :, 3:] = (rng.integers(-64, 64, size=3) / 16.0).astype(np.float32).reshape(3, 1, 1, 1)
    ints, floats = series_of(block, seg, labels, scale)
    trace = covariance_trace_np(block, seg, labels, scale)
    table = sr.structure_summary(ints, floats, ['a', 'b'], chains=1, cov_trace=trace)['structures']
    for row in table.values():
        assert abs(row['coherence'] - 1.0) <= 1e-12 and abs(row['n_eff'] - 1.0) <= 1e-12
    # independent voxels: Var(mean) = sigma^2 / voxels, so coherence ~ 1 / voxels (a ratio of two variance estimates from n records
    # each: the numerator is chi-square with 3 (n - 1) degrees of freedom, relative spread sqrt(2 / 33) = 0.25)
    white = rng.normal(size=(n, 3) + shape).astype(np.float32)
    ints, floats = series_of(white, seg, labels)
    trace = covariance_trace_np(white, seg, labels)
    table = sr.structure_summary(ints, floats, ['a', 'b'], chains=1, cov_trace=trace)['structures']
    for row in table.values():
        assert 0.3 / row['voxels'] < row['coherence'] < 2.5 / row['voxels'] and row['n_eff'] == 1.0 / row['coherence']
        assert row['coherence'] <= 1.0
    want = summary_np(ints, floats, ['a', 'b'], chains=1, cov_trace=trace)
    for name, row in table.items():
        for key, v in row.items():
            assert v == pytest.approx(want[name][key], rel=1e-9, abs=1e-12, nan_ok=True), (name, key)
    # covariance_trace: from the sums structure_map_stats would give of the three co-moment maps
    comoment = (white.astype(np.float64).var(axis=0, ddof=0) * n).astype(np.float32)
    ms = map_stats_np(comoment, seg, labels)
    got = sr.covariance_trace(ms['ints'], ms['floats'], n)
    assert np.allclose(got, trace, rtol=1e-5)
    assert np.isnan(sr.covariance_trace(ms['ints'], ms['floats'], 1)).all()


def test_summary_against_the_restatement_and_the_shared_split_rhat():
    shape = (5, 6, 7)
    labels = label_values(3)
    seg = label_volume('white', shape, labels, 4)  # every structure has voxels
    rng = np.random.default_rng(5)
    n, chains = 10, 2
    u = rng.normal(size=(n, 3) + shape).astype(np.float32)
    ints, floats = series_of(u, seg, labels, (1.0, 1.0, 1.0))
    got = sr.structure_summary(ints, floats, list('abc'), spacing=(1.5, 1.0, 2.0), chains=chains)
    want = summary_np(ints, floats, list('abc'), spacing=(1.5, 1.0, 2.0), chains=chains)
    assert got['records'] == n
    for name in 'abc':
        assert list(got['structures'][name]) == list(sr.MOTION_KEYS)
        for key in sr.MOTION_KEYS:
            assert got['structures'][name][key] == pytest.approx(want[name][key], rel=1e-9, abs=1e-12, nan_ok=True), (name, key)
        assert math.isfinite(got['structures'][name]['rhat_max'])  # 5 records per chain
    # fewer than 4 records per chain, or one chain: no R-hat
    assert math.isnan(sr.structure_summary(ints[:6], floats[:6], list('abc'), chains=2)['structures']['a']['rhat_max'])
    assert math.isnan(sr.structure_summary(ints, floats, list('abc'), chains=1)['structures']['a']['rhat_max'])
    # the helper is the one modes.py applies to the mode scores
    x = rng.normal(size=(3, 9))
    assert split_rhat_series(x) == pytest.approx(split_rhat_np(x), rel=1e-12)
    assert split_rhat_series(np.ones((2, 4))) == 1.0
    with pytest.raises(ValueError, match='records of'):
        sr.structure_summary(ints, floats, ['a'])


# ---------------------------------------------------------------- the option
def test_option_parsing():
    assert sr.structure_report_options(BASE) is None
    for off in (False, None):
        assert sr.structure_report_options({**BASE, 'structure_report': off}) is None
    assert sr.structure_report_options({**BASE, 'structure_report': True}) == {'period': 4, 'maps': True, 'save': True}
    assert sr.structure_report_options({**BASE, 'structure_report': {}}) == {'period': 4, 'maps': True, 'save': True}
    assert sr.structure_report_options({**BASE, 'structure_report': {'period': 3, 'maps': False}}) == {'period': 3, 'maps': False,
                                                                                                        'save': True}
    assert sr.structure_report_options({**BASE, 'structure_report': {'save': False}})['save'] is False


@pytest.mark.parametrize('opt,match', [
    ('yes', 'must be true, false or'),
    (3, 'must be true, false or'),
    ({'every': 2}, 'unknown keys'),
    ({'period': 2.0}, 'period must be an integer'),
    ({'period': True}, 'period must be an integer'),
    ({'period': 0}, 'the period must be >= 1'),
    ({'period': 13}, 'records no step'),
    ({'maps': 1}, 'structure_report.maps must be true or false'),
    ({'save': 'no'}, 'structure_report.save must be true or false'),
])
def test_option_refusals(opt, match):
    with pytest.raises(ValueError, match=match):
        sr.structure_report_options({**BASE, 'structure_report': opt})


def test_refusals_at_construction():
    class NoSegs:
        has_segs = False

    class Segs:
        has_segs = True
    cfg = {**BASE, 'structure_report': True}
    with pytest.raises(ValueError, match='trainer.structure_report needs the fixed segmentation, and the data loader \\(NoSegs\\) found no "segs"'):
        sr.structure_report_options(cfg, NoSegs(), {'a': 1})
    with pytest.raises(ValueError, match='trainer.structure_report needs structures'):
        sr.structure_report_options(cfg, Segs(), {})
    assert sr.structure_report_options(cfg, Segs(), {'a': 1})['period'] == 4
    assert sr.structure_report_options(BASE, NoSegs(), {}) is None  # off: nothing is asked of the data


def test_metric_names_and_registration():
    structures = {'left': 1, 'right': 2}
    cfg = {**BASE, 'structure_report': {'period': 2}}
    names = sr.structure_metric_names(cfg, structures)
    assert names[:2] == ['MCMC/structure/voxels/left', 'MCMC/structure/shift_mean_x/left']
    assert len(names) == 2 * len(sr.MOTION_KEYS) and not [n for n in names if 'coherence' in n]
    # the coherence needs the covariance with the SAME period
    assert not sr.with_coherence({**cfg, 'displacement_covariance': {'period': 4}})
    both = {**cfg, 'displacement_covariance': {'period': 2}}
    assert sr.with_coherence(both)
    names = sr.structure_metric_names(both, structures)
    assert len(names) == 2 * (len(sr.MOTION_KEYS) + 2) and names[-1] == 'MCMC/structure/n_eff/right'
    # registered by the config parser exactly when the option is on
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = json.load(open(os.path.join(root, 'configs', 'synthetic_ssd_l2_128_structures.json')))
    base = json.load(open(os.path.join(root, 'configs', 'synthetic_ssd_l2_128.json')))
    assert raw['trainer']['structure_report'] and raw['trainer']['displacement_covariance']
    assert {k: v for k, v in raw.items() if k not in ('trainer', 'name')} == {k: v for k, v in base.items() if k not in ('trainer', 'name')}
    assert {k: v for k, v in raw['trainer'].items() if k not in ('structure_report', 'displacement_covariance')} == base['trainer']
    on = ConfigParser.from_dict(raw, make_dirs=False)
    off = ConfigParser.from_dict(base, make_dirs=False)
    m_on, m_off = on.init_metrics(), off.init_metrics()
    assert not [m for m in m_off if m.startswith('MCMC/structure/')]
    assert [m for m in m_on if m.startswith('MCMC/structure/')] == sr.structure_metric_names(raw['trainer'], on.structures_dict)
    assert f'MCMC/structure/coherence/{next(iter(on.structures_dict))}' in m_on


def test_csv_round_trip(tmp_path):
    shape = (4, 5, 6)
    labels = label_values(2) + [4242]
    seg = label_volume('blocks', shape, labels[:2], 2)
    rng = np.random.default_rng(6)
    n, chains = 6, 2
    u = rng.normal(size=(n, 3) + shape).astype(np.float32)
    ints, floats = series_of(u, seg, labels)
    names = ['left', 'right', 'nowhere']
    summary = sr.structure_summary(ints, floats, names, chains=chains)
    ms = map_stats_np(rng.normal(size=(2,) + shape).astype(np.float32), seg, labels)
    rows = sr.structure_map_rows(ms['ints'], ms['floats'], ['split_rhat', 'ess'], names)
    sr.add_map_rows(summary, rows, ['split_rhat', 'ess'])
    assert summary['maps'] == ['split_rhat', 'ess']
    with pytest.raises(ValueError, match='rhat_max'):  # the map 'rhat' would replace the motion key rhat_max
        sr.add_map_rows(sr.structure_summary(ints, floats, names, chains=chains),
                        sr.structure_map_rows(ms['ints'], ms['floats'], ['rhat'], names), ['rhat'])
    header, table = sr.structures_csv(summary)
    sr.write_csv(tmp_path / 'structures.csv', header, table)
    got_header, got = sr.read_csv(tmp_path / 'structures.csv')
    assert got_header == header == ['structure'] + list(sr.MOTION_KEYS) + [f'{m}_{k}' for m in ('split_rhat', 'ess') for k in sr.MAP_KEYS]
    for line in got:
        want = summary['structures'][line[0]]
        for key, cell in zip(header[1:], line[1:]):
            assert (isinstance(cell, float) and math.isnan(cell) and math.isnan(want[key])) or cell == want[key], (line[0], key)
            assert type(cell) is type(want[key]), (key, cell)
    steps = [4, 6, 8]
    sheader, srows = sr.series_csv(ints, floats, names, steps, chains)
    sr.write_csv(tmp_path / 'series.csv', sheader, srows)
    got_header, got = sr.read_csv(tmp_path / 'series.csv')
    assert tuple(got_header) == sr.SERIES_COLUMNS and len(got) == n * len(names)
    series = sr.structure_series(ints, floats)
    for line in got:
        r, step, chain, name = line[:4]
        j = names.index(name)
        assert step == steps[r // chains] and chain == r % chains
        want = [*series['shift'][r, j], series['vol_ratio'][r, j], series['disp_mean'][r, j]]
        for cell, w in zip(line[4:9], want):
            assert (math.isnan(cell) and math.isnan(w)) or cell == w
        assert line[9] == ints[r, j, 1]
