"""Known-transformation validation on the host (no GPU): the numpy restatement of the two kernels (tests/_truth_calibration.py)
against linear algebra and a case with a known answer, the thresholds against scipy, the velocity generator, the summary and
every refusal of the option parser."""
import math

import numpy as np
import pytest

from ir_sgmcmc_amd import truth as T
from tests._truth_calibration import (calibrate_np, gaussian_case, rank_fractions_np, summary_np, update_np, velocity_np, welford_np)

LEVELS = (0.5, 0.9, 0.95)
N = 63


def _calibrated(records, truth, n, reference, rank_bins=8, mask=None):
    mean, M = welford_np(records)
    below, _, _, _ = update_np(records, truth, None, 0)
    edges, lv = T.calibration_thresholds(n, LEVELS, 20, reference)
    var_edges = T.default_var_edges(16)
    res = calibrate_np(mean, M, below, truth, n, (1, 1, 1), edges, lv, rank_bins, var_edges, 1e-3, mask)
    summary = T.calibration_summary(res['isummary'], res['fsummary'], res['pit_hist'], res['coverage'], res['rank_hist'],
                                    res['rel_ints'], res['rel_floats'], n, LEVELS, reference, var_edges)
    return res, summary


@pytest.fixture(scope='module')
def gaussian():
    records, truth = gaussian_case()
    return records, truth, _calibrated(records, truth, N, 'hotelling')


def test_mahalanobis_agrees_with_a_linear_solve():
    rng = np.random.default_rng(3)
    dims = (4, 5, 6)
    A = rng.standard_normal(dims + (3, 3))
    S = A @ np.swapaxes(A, -1, -2) + 0.5 * np.eye(3)  # well conditioned
    n, scale, f = 11, (1.5, 0.75, 2.0), 1e-3
    M = np.stack([S[..., a, b] for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]).astype(np.float32) * (n - 1)
    mean, truth = rng.standard_normal((3,) + dims).astype(np.float32), rng.standard_normal((3,) + dims).astype(np.float32)
    res = calibrate_np(mean, M, np.zeros((3,) + dims, dtype=np.uint16), truth, n, scale, [1.0], [1.0], 4, [1.0], f)
    s = np.asarray(scale)
    Mf = M.astype(np.float64)
    full = np.empty(dims + (3, 3))
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        full[..., a, b] = full[..., b, a] = s[a] * s[b] * Mf[k] / (n - 1)
    full += f * f * np.eye(3)
    delta = np.moveaxis(s.reshape(3, 1, 1, 1) * (mean.astype(np.float64) - truth.astype(np.float64)), 0, -1)
    ref = np.einsum('...a,...a->...', delta, np.linalg.solve(full, delta[..., None])[..., 0])
    assert np.max(np.abs(res['d2'] - ref) / ref) < 1e-10
    assert not res['raised'].any() and res['finite'].all()
    np.testing.assert_allclose(res['v'], np.trace(full, axis1=-2, axis2=-1), rtol=1e-14)


def test_thresholds_agree_with_scipy():
    from scipy import stats
    p = np.asarray([0.05, 0.5, 0.9, 0.95, 0.999])
    np.testing.assert_allclose(T.d2_quantile(p, N, 'chi2'), stats.chi2.ppf(p, 3), rtol=1e-13)
    for n in (6, 20, N, 1000):
        ref = (1 + 1 / n) * 3 * (n - 1) / (n - 3) * stats.f.ppf(p, 3, n - 3)
        np.testing.assert_allclose(T.d2_quantile(p, n, 'hotelling'), ref, rtol=1e-13)
    # n -> infinity: the Hotelling law tends to chi^2_3 from above
    assert np.all(T.d2_quantile(p, 10 ** 6, 'hotelling') > T.d2_quantile(p, 0, 'chi2'))
    np.testing.assert_allclose(T.d2_quantile(p, 10 ** 6, 'hotelling'), stats.chi2.ppf(p, 3), rtol=1e-4)
    edges, lv = T.calibration_thresholds(N, LEVELS, 20)
    assert len(edges) == 19 and np.all(np.diff(edges) > 0) and len(lv) == 3
    assert T.expected_scale(N) == pytest.approx(math.sqrt((1 + 1 / N) * (N - 1) / (N - 5)), rel=1e-15)
    assert T.expected_scale(N, 'chi2') == 1.0 and math.isnan(T.expected_scale(5))
    with pytest.raises(ValueError, match='n >= 4'):
        T.d2_quantile(0.5, 3)
    with pytest.raises(ValueError, match="'gauss'"):
        T.d2_quantile(0.5, 10, 'gauss')


def test_a_calibrated_gaussian_posterior_is_found_calibrated(gaussian):
    """12 x 10 x 14 voxels, 63 iid records, default_rng(20261020) drawn as gaussian_case draws them: Hotelling coverage 0.499 /
    0.907 / 0.957, 8-bin rank chi^2 9.3 / 6.4 / 6.8 against 24.3, scale factor 1.037 / 1.042"""
    _, _, (res, s) = gaussian
    V = s['voxels']
    assert V == 12 * 10 * 14 and s['nonfinite_voxels'] == 0 and s['raised_voxels'] == 0
    for lv in LEVELS:
        row = s['coverage'][T.coverage_key(lv)]
        print(lv, row['observed'])
        assert abs(row['observed'] - lv) <= 4 * math.sqrt(lv * (1 - lv) / V)
    from scipy import stats
    critical = stats.chi2.ppf(0.999, 7)
    for axis in 'xyz':
        print(axis, s[f'rank_chi2_{axis}'], critical)
        assert s[f'rank_chi2_{axis}'] < critical
    print(s['scale_factor_raw'], s['scale_factor_expected'], s['scale_factor'])
    assert abs(s['scale_factor'] - 1) < 0.03
    assert s['pit_chi2'] < stats.chi2.ppf(0.999, 19)
    # the summary restates what the restatement's own few lines give
    ref = summary_np(res, N, LEVELS)
    assert [s['coverage'][T.coverage_key(lv)]['observed'] for lv in LEVELS] == ref['coverage']
    np.testing.assert_allclose([s[f'rank_chi2_{a}'] for a in 'xyz'], ref['rank_chi2'], rtol=1e-12)
    for key in ('scale_factor', 'pit_chi2', 'rmse', 'mean', 'max'):
        assert s[key] == pytest.approx(ref[key], rel=1e-12)
    assert sum(s['pit_hist']) == V and all(sum(h) == V for h in s['rank_hist'])
    assert sum(r['count'] for r in s['reliability']) == V and 0 <= s['ence'] < 0.2


def test_chi2_thresholds_under_cover_at_63_records(gaussian):
    records, truth, (_, hot) = gaussian
    _, chi = _calibrated(records, truth, N, 'chi2')
    for lv in LEVELS:
        key = T.coverage_key(lv)
        assert chi['coverage'][key]['observed'] < hot['coverage'][key]['observed']
    assert chi['coverage']['90']['observed'] < 0.9 - 0.01 < hot['coverage']['90']['observed']
    assert chi['scale_factor'] == pytest.approx(hot['scale_factor_raw'], rel=1e-15) and chi['scale_factor'] > 1.03


def test_an_under_dispersed_posterior_is_found(gaussian):
    """the same records, the truth doubled: scale factor 2.059 / 1.042 = 1.976, coverage 0.099 / 0.353 / 0.449"""
    records, _, _ = gaussian
    _, truth2 = gaussian_case(truth_factor=2.0)
    _, s = _calibrated(records, truth2, N, 'hotelling')
    print(s['scale_factor'])
    assert abs(s['scale_factor'] - 2) < 0.05 * 2
    for lv in LEVELS:
        assert s['coverage'][T.coverage_key(lv)]['observed'] < lv
    assert max(s[f'z_rms_{a}'] for a in 'xyz') > 1.5


def test_rank_histogram_expectation_is_exact_for_unequal_bins():
    for n, Br in ((63, 16), (63, 8), (10, 4), (12, 5), (65535, 64), (7, 16)):
        frac = T.rank_expected_fractions(n, Br)
        assert frac.sum() == pytest.approx(1.0, abs=1e-15)
        np.testing.assert_array_equal(frac, rank_fractions_np(n, Br))
        if (n + 1) % Br == 0:
            assert np.all(frac == 1.0 / Br)
        else:
            assert frac.min() < frac.max()
    # n + 1 = 11 ranks in 4 bins: r * 4 // 11 -> 3, 3, 3, 2 ranks
    np.testing.assert_array_equal(T.rank_expected_fractions(10, 4) * 11, [3, 3, 3, 2])
    # uniform ranks reproduce the expectation exactly: chi^2 = 0 although the bins differ
    n, Br, reps = 12, 5, 7
    below = np.tile(np.arange(n + 1), reps)
    hist = np.bincount(below * Br // (n + 1), minlength=Br)
    s = T.calibration_summary([len(below), 0, 0], [0.0] * 9, [len(below)], [0], [hist, hist, hist], [len(below)], [[1.0, 1.0]], n,
                              [0.5], 'chi2', [])
    assert s['rank_chi2_x'] == 0.0 and s['rank_expected'] == (T.rank_expected_fractions(n, Br) * len(below)).tolist()


def test_update_restatement_counts_and_specials():
    t = np.zeros((3, 2, 2, 2), dtype=np.float32)
    u = np.zeros((2, 3, 2, 2, 2), dtype=np.float32)
    u[0, 0, 0, 0, 0] = -1.0          # below
    u[1, 0, 0, 0, 0] = np.nan        # not below, non-finite
    u[0, 1, 0, 0, 1] = np.inf        # not below, non-finite
    u[1, 2, 1, 1, 1] = -np.inf       # below, non-finite
    below, ints, floats, _ = update_np(u, t, None, 0)
    assert below[0, 0, 0, 0] == 1 and below[1, 0, 0, 1] == 0 and below[2, 1, 1, 1] == 1 and below.sum() == 2
    assert ints.tolist() == [[8, 1], [8, 2]] and floats[0].tolist() == [1.0, 1.0, 1.0] and floats[1].tolist() == [0.0, 0.0, 0.0]
    again, _, _, _ = update_np(u, t, below, 2)
    assert again.sum() == 4


def test_velocity_generator():
    dims = (9, 12, 17)
    v = T.simulate_velocity(dims, 5, 3.0)
    assert v.dtype == np.float32 and v.shape == (3,) + dims
    np.testing.assert_array_equal(v, T.simulate_velocity(dims, 5, 3.0))
    np.testing.assert_array_equal(v, velocity_np(dims, 5, 3.0))
    assert not np.array_equal(v, T.simulate_velocity(dims, 6, 3.0))
    for amplitude in (3.0, 0.1, 2.5e-3, 7.3):
        w = T.simulate_velocity(dims, 11, amplitude, modes=3, max_wavenumber=3)
        assert np.abs(w).max() == np.float32(amplitude)
        for axis in (1, 2, 3):
            assert not np.take(w, [0, -1], axis=axis).any()
    assert not T.simulate_velocity(dims, 5, 0.0).any()
    # smooth: wavenumbers <= 2 over 17 samples change by a fraction of the amplitude per voxel
    assert np.abs(np.diff(v, axis=3)).max() < 0.9 * 3.0
    for bad in (dict(amplitude=-1.0), dict(amplitude=float('nan')), dict(modes=0), dict(max_wavenumber=0)):
        with pytest.raises(ValueError):
            T.simulate_velocity(dims, 0, **{'amplitude': 1.0, **bad})
    with pytest.raises(ValueError, match='dims'):
        T.simulate_velocity((1, 4, 4), 0, 1.0)


def test_read_truth_round_trip(tmp_path):
    from ir_sgmcmc_amd.utils.imageio import write_vtk_field
    dims = (4, 5, 6)
    field = np.random.default_rng(0).standard_normal((3,) + dims).astype(np.float32)
    write_vtk_field(field, tmp_path / 't.vtk', (2.0, 2.0, 2.0))
    np.testing.assert_array_equal(T.read_truth(tmp_path / 't.vtk', dims, 'voxels'), field)
    np.testing.assert_array_equal(T.read_truth(tmp_path / 't.vtk', dims, 'mm', (2.0, 2.0, 2.0)), field / np.float32(2))
    assert T.fingerprint(field) == T.fingerprint(field.copy()) != T.fingerprint(field + 1)
    with pytest.raises(ValueError, match=r'\(4, 5, 6\) grid'):
        T.read_truth(tmp_path / 't.vtk', (4, 5, 7))
    with pytest.raises(ValueError, match="'furlongs'"):
        T.read_truth(tmp_path / 't.vtk', dims, 'furlongs')
    field[0, 0, 0, 0] = np.nan
    write_vtk_field(field, tmp_path / 'n.vtk')
    with pytest.raises(ValueError, match='1 non-finite'):
        T.read_truth(tmp_path / 'n.vtk', dims)


# ---------------------------------------------------------------- the option parser
BASE = {'no_samples_MCMC': 100, 'log_period_MCMC': 10, 'no_chains': 2, 'MCMC': True}
SIM = {'source': 'simulate'}


def _cfg(truth, **extra):
    return {**BASE, 'truth': truth, **extra}


def test_option_off_and_defaults():
    for off in (None, False):
        assert T.truth_options(_cfg(off)) is None
    assert T.truth_options(dict(BASE)) is None
    o = T.truth_options(_cfg(SIM))
    assert o == {'period': 10, 'source': 'simulate', 'seed': 0, 'amplitude': 2.0, 'modes': 6, 'max_wavenumber': 2, 'noise': 0.0,
                 'path': None, 'unit': 'voxels', 'levels': (0.5, 0.9, 0.95), 'pit_bins': 20, 'rank_bins': 16, 'reliability_bins': 16,
                 'std_floor': 1e-3, 'reference': 'hotelling', 'save': True}
    o = T.truth_options(_cfg({'source': 'file', 'path': 'truth.vtk', 'unit': 'mm', 'period': 5, 'levels': [0.8], 'reference': 'chi2'}))
    assert (o['path'], o['unit'], o['period'], o['levels'], o['reference']) == ('truth.vtk', 'mm', 5, (0.8,), 'chi2')
    names = T.truth_metric_names(T.truth_options(_cfg(SIM)))
    assert 'truth/initial/rmse' in names and 'MCMC/truth/coverage_95' in names and 'MCMC/truth/rank_chi2_z' in names


@pytest.mark.parametrize('truth, word', [
    (True, 'source'), ('simulate', "'simulate'"), ({}, 'source'), ({'source': 'guess'}, "'guess'"),
    ({**SIM, 'colour': 1}, 'colour'), ({**SIM, 'path': 'a.vtk'}, "'path'"), ({'source': 'file', 'path': 'a.vtk', 'seed': 1}, "'seed'"),
    ({'source': 'file'}, 'path'), ({'source': 'file', 'path': ''}, 'path'), ({'source': 'file', 'path': 'a.vtk', 'unit': 'cm'}, "'cm'"),
    ({**SIM, 'seed': -1}, '-1'), ({**SIM, 'seed': 1.5}, '1.5'), ({**SIM, 'seed': True}, 'True'),
    ({**SIM, 'amplitude': -2.0}, '-2.0'), ({**SIM, 'amplitude': 'big'}, "'big'"), ({**SIM, 'amplitude': float('inf')}, 'inf'),
    ({**SIM, 'modes': 0}, 'modes'), ({**SIM, 'modes': 2.5}, '2.5'), ({**SIM, 'max_wavenumber': 0}, 'max_wavenumber'),
    ({**SIM, 'noise': -0.1}, '-0.1'), ({**SIM, 'period': 0}, 'period'), ({**SIM, 'period': 2.5}, '2.5'), ({**SIM, 'period': 200}, 'no step'),
    ({**SIM, 'levels': []}, 'levels'), ({**SIM, 'levels': [0.9, 0.5]}, r'\[0.9, 0.5\]'), ({**SIM, 'levels': [0.5, 1.0]}, '1.0'),
    ({**SIM, 'levels': 0.9}, 'levels'), ({**SIM, 'levels': [0.1 * i for i in range(1, 10)]}, '9'),
    ({**SIM, 'pit_bins': 1}, 'pit_bins'), ({**SIM, 'pit_bins': 65}, '65'), ({**SIM, 'rank_bins': 1}, 'rank_bins'),
    ({**SIM, 'rank_bins': 100}, '100'), ({**SIM, 'reliability_bins': 0}, 'reliability_bins'), ({**SIM, 'reliability_bins': 33}, '33'),
    ({**SIM, 'std_floor': 0.0}, '0.0'), ({**SIM, 'std_floor': 1e-200}, '1e-200'), ({**SIM, 'std_floor': float('nan')}, 'nan'),
    ({**SIM, 'reference': 'student'}, "'student'"), ({**SIM, 'save': 1}, 'save'),
])
def test_option_refusals(truth, word):
    with pytest.raises(ValueError, match=word):
        T.truth_options(_cfg(truth))


def test_option_refused_combinations():
    with pytest.raises(ValueError, match='MCMC is false'):
        T.truth_options(_cfg(SIM, MCMC=False))
    with pytest.raises(ValueError, match='4 records, at least 6'):
        T.truth_options(_cfg({**SIM, 'period': 50}))
    assert T.truth_options(_cfg({**SIM, 'period': 50, 'reference': 'chi2'}))['period'] == 50
    with pytest.raises(ValueError, match='65535'):
        T.truth_options({**BASE, 'no_samples_MCMC': 40000, 'truth': {**SIM, 'period': 1}})
    with pytest.raises(ValueError, match='affine_init'):
        T.truth_options(_cfg(SIM, affine_init={'model': 'rigid'}))
    with pytest.raises(ValueError, match='affine_init'):
        T.truth_options(_cfg({'source': 'file', 'path': 'a.vtk'}, affine_init={'model': 'rigid'}))
    for key in ('native_resolution', 'native_posterior', 'landmarks'):
        with pytest.raises(ValueError, match=key):
            T.truth_options(_cfg(SIM, **{key: True}))
        assert T.truth_options(_cfg({'source': 'file', 'path': 'a.vtk'}, **{key: True})) is not None
    with pytest.raises(ValueError, match='t1.nii'):
        T.truth_options(_cfg(SIM, image_posterior={'volumes': [{'name': 't1', 'path': 't1.nii'}]}))
    assert T.truth_options(_cfg(SIM, image_posterior=True)) is not None
    assert T.truth_options(_cfg(SIM, image_posterior={'volumes': []})) is not None


def test_summary_of_an_empty_mask_and_the_floor():
    s = T.calibration_summary([0, 0, 0], [0.0, 0.0, -np.inf, 0.0, -np.inf, 0.0, 0.0, 0.0, 0.0], [0] * 4, [0], np.zeros((3, 4)), [0, 0],
                              np.zeros((2, 2)), 10, [0.9], 'hotelling', [1.0])
    assert math.isnan(s['rmse']) and math.isnan(s['scale_factor']) and math.isnan(s['ence']) and math.isnan(s['pit_ks'])
    assert math.isnan(s['coverage']['90']['observed']) and not s['below_floor']
    s = T.calibration_summary([10, 0, 0], [1.0, 0.2, 0.3, 30.0, 5.0, 4.0, 10.0, 10.0, 10.0], [5, 5], [9], np.full((3, 2), 5), [10],
                              [[4.0, 0.2]], 10, [0.9], 'chi2', [], initial={'mean': 2.0, 'rmse': 2.5, 'max': 3.0},
                              floor={'floor_mean': 0.5, 'floor_max': 0.9})
    assert s['mean'] == 0.1 and s['below_floor'] and s['initial_rmse'] == 2.5 and s['floor_max'] == 0.9
    assert s['scale_factor'] == 1.0 and s['z_rms_x'] == 1.0 and s['coverage']['90']['observed'] == 0.9
    assert s['ence'] == pytest.approx(abs(math.sqrt(0.4) - math.sqrt(0.02)) / math.sqrt(0.4))
    header, rows = T.calibration_csv(s)
    assert header[:3] == ['table', 'bin', 'count'] and {r[0] for r in rows} == {'pit', 'rank_x', 'rank_y', 'rank_z', 'reliability', 'coverage'}
    header, rows = T.series_csv(np.asarray([[4, 0], [4, 1]]), np.asarray([[2.0, 4.0, 1.0], [3.0, 3.0, 1.0]]), [7], 2)
    assert header == list(T.SERIES_COLUMNS) and rows[1][:3] == ['1', '7', '1'] and float(rows[0][4]) == 1.0 and float(rows[1][3]) == 1.0
