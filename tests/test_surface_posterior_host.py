"""Host side of the surface posterior (no GPU): the known answers and the float32 evaluation of the restatement
(tests/_surface_posterior.py), whose docstring derives the tolerances; the options parser; surface_summary; the refusals of the
two entry points that happen before any HIP call."""
import ctypes as C
import math

import numpy as np
import pytest

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.diagnostics import (SURFACE_DEFAULTS, surface_coverage_key, surface_metric_names, surface_posterior_options,
                                       surface_summary)
from tests import _surface_posterior as SP
from tests._report import check

LEVELS = (0.5, 0.9, 0.95)


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize('spacing', SP.SPACINGS)
@pytest.mark.parametrize('a,b', [(4, 7), (7, 4)])
def test_half_spaces_give_the_signed_offset(a, b, spacing):
    f, m = SP.half_spaces((3, 4, 12), a, b)
    s = SP.samples(f, m, [16], spacing)[0]
    on = SP.fixed_contours(f, [16]) == 0
    assert on.sum() == 3 * 4 and np.array_equal(np.argwhere(on)[:, 2], np.full(12, a - 1))
    assert np.array_equal(s[on], np.full(12, (a - b) * spacing[0])) and np.isnan(s[~on]).all()


@pytest.mark.parametrize('spacing', SP.SPACINGS)
def test_single_voxels_give_the_positive_distance(spacing):
    p, q = (1, 2, 3), (4, 0, 5)
    f, m = SP.single_voxels((6, 5, 7), p, q)
    s = SP.samples(f, m, [10, 11], spacing)[0]
    assert np.isfinite(s).sum() == 1 and s[p] == SP.point_distance(p, q, spacing) > 0


def test_identical_maps_give_zero_and_a_missing_label_no_sample():
    f, moving, _ = SP.case_maps((5, 7, 9), 2)
    s = SP.samples(f, np.stack([f, np.where(f == 10, 0, f)]), SP.LABELS3, (1.0, 1.0, 1.0))
    li = SP.fixed_contours(f, SP.LABELS3)
    assert (s[0][li >= 0] == 0.0).all() and not np.signbit(s[0][li >= 0]).any()
    assert np.isnan(s[1][li == 0]).all() and (s[1][li > 0] == 0.0).all()


def test_equal_records_leave_the_sample_and_no_spread():
    s = np.array([[[[1.25, -3.5, np.nan]]]])
    mean, m2, count = SP.welford([np.repeat(s, 3, axis=0)] * 2, np.float32)
    assert np.array_equal(count, [[[6, 6, 0]]]) and np.array_equal(mean, np.float32([[[1.25, -3.5, 0.0]]])) and not m2.any()


# ------------------------------------------------------------------------------------------------ the bounds are reachable
@pytest.mark.parametrize('dims', SP.SHAPES)
@pytest.mark.parametrize('C', SP.CHAINS)
def test_float32_evaluation_stays_inside_the_tolerances(dims, C):
    fixed, _, mask = SP.case_maps(dims, C)
    for spacing in SP.SPACINGS:
        ref = SP.case_reference(dims, C, spacing)
        name = f'surface_posterior_fp32_numpy/{dims}/C{C}/{spacing}'
        assert (ref['count'] >= 2).any()
        mean, m2, count = SP.welford(ref['s'], np.float32)
        SP.check_state(name, check, mean, m2, count, ref, ref['S'])
        off = ref['count'] == 0
        assert not mean[off].any() and not m2[off].any()
        bias, std = SP.maps(mean, m2, count)
        SP.check_maps(name, check, bias, std, ref, ref['S'])
        for mk in (None, mask):
            got_i, got_f = SP.summary(bias, std, count, fixed, SP.LABELS3, LEVELS, mk)
            SP.check_summary(name, check, got_i, got_f, bias, std, ref, fixed, SP.LABELS3, LEVELS, ref['S'], mk)


def test_tolerances_grow_with_the_count_and_the_scale():
    K = np.arange(0, 10)
    e, f = SP.mean_tol(K, 3.0), SP.m2_tol(K, 3.0)
    assert e[0] == 0 and f[0] == 0 and (np.diff(e) > 0).all() and (np.diff(f) > 0).all()
    assert e[1] == SP.U * 3.0 * 6.0 and f[1] == SP.U * 9.0 * (4 * 6.0 + 17.0)
    assert np.allclose(SP.mean_tol(K, 6.0), 2 * e) and np.allclose(SP.m2_tol(K, 6.0), 4 * f)
    assert SP.std_tol(np.array([2]), 3.0, np.array([0.0]))[0] == pytest.approx(math.sqrt(f[2]) * (1 + 4 * SP.U))


# ------------------------------------------------------------------------------------------------ options
BASE = {'no_samples_MCMC': 80, 'log_period_MCMC': 10, 'no_chains': 2}


def test_options_accepts():
    assert surface_posterior_options(BASE) is None
    for off in (False, None):
        assert surface_posterior_options({**BASE, 'surface_posterior': off}) is None
    default = {'period': 10, 'coverage': (0.5, 0.9, 0.95), 'save': True}
    assert surface_posterior_options({**BASE, 'surface_posterior': True}) == default == {'period': 10, **SURFACE_DEFAULTS}
    assert surface_posterior_options({**BASE, 'surface_posterior': {}}) == default
    assert surface_posterior_options({**BASE, 'surface_posterior': {'period': 3}}) == {**default, 'period': 3}
    assert surface_posterior_options({**BASE, 'surface_posterior': {'coverage': []}})['coverage'] == ()
    assert surface_posterior_options({**BASE, 'surface_posterior': {'coverage': [0.1, 0.2, 0.3, 0.999]}})['coverage'] == (0.1, 0.2, 0.3, 0.999)
    assert surface_posterior_options({**BASE, 'surface_posterior': {'save': False, 'period': 80}}) == {**default, 'save': False, 'period': 80}


@pytest.mark.parametrize('opt', [1, 'yes', [], {'perod': 2}, {'period': 0}, {'period': -1}, {'period': 2.0}, {'period': True},
                                 {'period': 81}, {'save': 1}, {'coverage': 0.5}, {'coverage': '0.5'}, {'coverage': [0.0]},
                                 {'coverage': [1.0]}, {'coverage': [0.9, 0.5]}, {'coverage': [0.5, 0.5]}, {'coverage': [True]},
                                 {'coverage': [0.1, 0.2, 0.3, 0.4, 0.5]}, {'coverage': [float('nan')]}])
def test_options_refuses(opt):
    with pytest.raises(ValueError, match='surface_posterior'):
        surface_posterior_options({**BASE, 'surface_posterior': opt})


def test_options_record_ceiling():
    big = {'no_samples_MCMC': 2 ** 31, 'log_period_MCMC': 1, 'no_chains': 2}
    with pytest.raises(ValueError, match='surface_posterior.*at most 2147483647'):
        surface_posterior_options({**big, 'surface_posterior': True})
    assert surface_posterior_options({**big, 'no_chains': 1, 'surface_posterior': {'period': 2}})['period'] == 2


def test_metric_names():
    assert [surface_coverage_key(q) for q in (0.5, 0.9, 0.95, 0.999)] == ['coverage_50', 'coverage_90', 'coverage_95', 'coverage_99.9']
    names = surface_metric_names({'coverage': (0.5, 0.95)}, ['a', 'b'])
    assert names == [f'MCMC/surface/{k}/{s}' for k in ('bias', 'abs_bias', 'std', 'coverage_50', 'coverage_95') for s in ('a', 'b')]


def test_init_metrics_names_the_surfaces_only_when_on(tmp_path):
    import copy
    import json
    import os
    from ir_sgmcmc_amd.parse_config import ConfigParser
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = json.load(open(os.path.join(root, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)

    def metrics(**over):
        c = copy.deepcopy(cfg)
        c['trainer'].update(over)
        return ConfigParser.from_dict(c, timestamp='t', make_dirs=False)

    off, on = metrics(), metrics(surface_posterior={'coverage': [0.9]})
    added = surface_metric_names({'coverage': (0.9,)}, on.structures_dict)
    m_off, m_on = off.init_metrics(), on.init_metrics()
    assert not [k for k in m_off if '/surface/' in k]
    assert [k for k in m_on if k not in added] == m_off and [k for k in m_on if k in added] == added


# ------------------------------------------------------------------------------------------------ surface_summary
def test_surface_summary_on_hand_made_columns():
    isum = [[10, 8, 4, 2, 3, 4, 0], [5, 0, 0, 0, 0, 0, 0], [3, 3, 0, 0, 0, 0, 0]]
    fsum = [[-4.0, 12.0, 32.0, 3.5, 2.0, 0.75], [0.0, 0.0, 0.0, -math.inf, 0.0, -math.inf], [1.5, 1.5, 0.75, 0.5, 0.0, -math.inf]]
    s = surface_summary(isum, fsum, ['a', 'empty', 'once'], (0.5, 0.9, 0.95), 6)
    assert s['records'] == 6 and list(s['structures']) == ['a', 'empty', 'once']
    a = s['structures']['a']
    assert a == {'bias': -0.5, 'abs_bias': 1.5, 'rms_bias': 2.0, 'max_abs_bias': 3.5, 'std': 0.5, 'max_std': 0.75, 'coverage_50': 0.5,
                 'coverage_90': 0.75, 'coverage_95': 1.0, 'contour_voxels': 10, 'sampled_voxels': 8, 'spread_voxels': 4}
    e = s['structures']['empty']
    assert (e['contour_voxels'], e['sampled_voxels'], e['spread_voxels']) == (5, 0, 0)
    assert all(math.isnan(e[k]) for k in e if not k.endswith('_voxels'))
    o = s['structures']['once']  # a sample, never two: the bias is defined, the spread and the coverage are not
    assert (o['bias'], o['abs_bias'], o['rms_bias'], o['max_abs_bias']) == (0.5, 0.5, 0.5, 0.5)
    assert all(math.isnan(o[k]) for k in ('std', 'max_std', 'coverage_50', 'coverage_90', 'coverage_95'))
    assert 'coverage_50' not in surface_summary(isum, fsum, ['a', 'b', 'c'], (), 6)['structures']['a']


# ------------------------------------------------------------------------------------------------ refusals before any HIP call
@pytest.mark.parametrize('fn,bad,message', SP.abi_refusals())
def test_abi_refusals(fn, bad, message):
    SP.assert_refused(fn, bad, message)
