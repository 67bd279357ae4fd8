"""Landmark propagation on the host (no GPU): the derived bound of tests/_landmarks.py against a float32 evaluation of the
reference in the kernel's rounding order, the exact cases, the closed form of pit, the option parser, the landmark files, the
grid geometry, the synthetic landmarks and the point-set writer."""
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import diagnostics as DG
from ir_sgmcmc_amd import landmarks as LM
from ir_sgmcmc_amd.data_loader import synthetic
from ir_sgmcmc_amd.native import NativeGrid
from ir_sgmcmc_amd.utils.imageio import write_vtk_points
from tests import _landmarks as R
from tests._exact_cases import EXACT_DIMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the bound
def test_float32_evaluation_stays_inside_the_derived_bound_and_the_bound_is_not_slack():
    worst = 0.0   # the largest observed error / bound over every case of the GPU test
    for dims in R.SMOOTH_DIMS:
        for C in R.SMOOTH_CHAINS:
            for K in R.SMOOTH_K:
                pts, field, offset = R.smooth_case(dims, C, K)
                s32, s64 = R.sample(pts, field, np.float32), R.sample(pts, field, np.float64)
                bound = R.sample_bound(field)
                err = float(np.abs(s32.astype(np.float64) - s64).max())
                assert err <= bound, (dims, C, K, err, bound)
                worst = max(worst, err / bound)
                m32 = R.mapped(s32, R.SMOOTH_SCALE, offset, np.float32)
                m64 = R.mapped(s64, R.SMOOTH_SCALE, offset, np.float64)
                mb = R.mapped_bound(field, R.SMOOTH_SCALE, offset, m64)
                merr = np.abs(m32.astype(np.float64) - m64).max(axis=(0, 1))
                assert (merr <= mb).all(), (dims, C, K, merr, mb)
    print(f'largest float32 error over the smooth cases: {worst:.3f} of the bound')
    assert 0.1 <= worst <= 1.0, f'largest observed error is {worst:.4f} of the derived bound (wanted within [0.1, 1])'


def test_the_bound_has_the_stated_form():
    field = R.smooth_field(2, (5, 6, 7), 1)
    L, big = R.adjacent_difference(field), float(np.abs(field).max())
    assert R.sample_bound(field) == R.SECOND_ORDER * R.U * (10 * big + 6 * 6 * L) and L > 0 and big == pytest.approx(R.AMPLITUDE)


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize('dims', EXACT_DIMS)
def test_exact_cases_agree_bit_for_bit_in_float32_and_float64(dims):
    pts, field, scale, offset = R.exact_case(dims)
    assert len(pts) == (30 if dims == (2, 3, 5) else 257)
    s32, s64 = R.sample(pts, field, np.float32), R.sample(pts, field, np.float64)
    assert np.array_equal(s32.astype(np.float64), s64)
    m32, m64 = R.mapped(s32, scale, offset, np.float32), R.mapped(s64, scale, offset, np.float64)
    assert np.array_equal(m32.astype(np.float64), m64)
    # the case holds what it promises: corners, points outside the box, points on the last voxel of every axis
    D, H, W = dims
    idx = [(pts[:, c].astype(np.float64) + 1) / 2 * (n - 1) for c, n in enumerate((W, H, D))]
    assert all((i == n - 1).any() and (i == 0).any() for i, n in zip(idx, (W, H, D)))
    if dims != (2, 3, 5):
        assert all((i < 0).any() and (i > n - 1).any() and (i % 1 != 0).any() for i, n in zip(idx, (W, H, D)))
    else:   # a voxel centre returns the stored value
        z, y, x = (np.rint(idx[2]).astype(int), np.rint(idx[1]).astype(int), np.rint(idx[0]).astype(int))
        assert np.array_equal(s32, field[:, :, z, y, x].transpose(0, 2, 1))


def test_reference_sampler_matches_grid_sample_and_clamps():
    pts, field, _ = R.smooth_case((5, 6, 7), 3, 65)
    want = torch.nn.functional.grid_sample(torch.from_numpy(field).double(), torch.from_numpy(pts).double().view(1, 1, 1, -1, 3)
                                           .expand(3, -1, -1, -1, -1), mode='bilinear', padding_mode='border', align_corners=True)
    got = R.sample(pts, field, np.float64)
    assert np.abs(got - want[:, :, 0, 0].permute(0, 2, 1).numpy()).max() < 1e-13
    bad = pts.copy()
    bad[3, 1], bad[7, 0], bad[9, 2] = np.nan, np.inf, -np.inf
    out = R.sample(bad, field, np.float32)
    rows = np.isnan(out).all(axis=(0, 2))
    assert rows.sum() == 3 and rows[[3, 7, 9]].all() and np.array_equal(out[:, ~rows], R.sample(pts, field, np.float32)[:, ~rows])


# ---------------------------------------------------------------- closed form of pit
def test_pit_closed_form_matches_the_integrated_density():
    """F3(x) against the chi-square(3) density sqrt(x) exp(-x/2) / sqrt(2 pi), integrated by Simpson's rule after x = t^2
    (the integrand 2 t^2 exp(-t^2 / 2) / sqrt(2 pi) is smooth at 0)"""
    for x in (0.0, 0.05, 0.5, 1.0, 2.366, 7.815, 20.0):
        top, n = math.sqrt(x), 4000
        t = np.linspace(0.0, top, n + 1)
        f = 2.0 * t * t * np.exp(-t * t / 2.0) / math.sqrt(2.0 * math.pi)
        simpson = (top / n / 3.0) * (f[0] + f[-1] + 4.0 * f[1:-1:2].sum() + 2.0 * f[2:-1:2].sum()) if x > 0 else 0.0
        assert abs(R.chi2_cdf3(x) - simpson) < 1e-12, x
    assert abs(R.chi2_cdf3(2.366) - 0.5) < 1e-4 and abs(R.chi2_cdf3(7.815) - 0.95) < 1e-4   # tabulated quantiles
    density = lambda x: math.sqrt(x) * math.exp(-x / 2) / math.sqrt(2 * math.pi)
    assert max(density(x) for x in np.linspace(0, 10, 100001)) < R.CHI2_3_MAX_DENSITY


def test_reference_recorder_on_a_hand_checked_case():
    """four samples (+-2,0,0), (0,+-1,0) around the origin, target (0,0,3): mean 0, S = diag(8/3, 2/3, 0), every e = sqrt(13) or
    sqrt(10)"""
    rec = [np.array([[[2, 0, 0]], [[-2, 0, 0]]], dtype=np.float32), np.array([[[0, 1, 0]], [[0, -1, 0]]], dtype=np.float32)]
    target = np.array([[0, 0, 3]], dtype=np.float32)
    ref = R.finalize(R.update(rec, target), target)
    t = ref['table'][0]
    e = np.array([math.sqrt(13)] * 2 + [math.sqrt(10)] * 2)
    assert t[0] == 4 and t[1] == pytest.approx(e.mean()) and t[2] == pytest.approx(e.std(ddof=1)) and t[3] == pytest.approx(e.max())
    assert t[4] == pytest.approx(3.0) and t[5:8] == pytest.approx([math.sqrt(8 / 3), math.sqrt(2 / 3), 0.0], abs=1e-12)
    assert np.isnan(t[8]) and np.isnan(t[9]) and ref['isummary'] == [1, 0, 0]
    # full rank: m = r' S^-1 r
    rec.append(np.array([[[0, 0, 1.5]], [[0, 0, -1.5]]], dtype=np.float32))
    ref = R.finalize(R.update(rec, target), target)
    assert ref['table'][0, 8] == pytest.approx(9.0 / (4.5 / 5)) and ref['table'][0, 9] == pytest.approx(R.chi2_cdf3(10.0))
    # a NaN sample is skipped and not counted
    rec.append(np.array([[[np.nan, 0, 0]], [[1, 1, 1]]], dtype=np.float32))
    assert R.finalize(R.update(rec, target), target)['table'][0, 0] == 7


def test_landmark_summary_host_half():
    table = np.full((5, 10), np.nan)
    table[:, 0] = [10, 10, 10, 0, 3]
    table[:4, 4], table[:4, 5], table[:4, 9] = [1.0, 2.0, 4.0, np.nan], [0.5, 1.0, 2.0, np.nan], [0.2, 0.6, 0.97, np.nan]
    table[4, 4], table[4, 5] = 3.0, 1.5
    table[[0, 1, 2, 4], 1], table[[0, 1, 2, 4], 3] = 1.5, [2, 3, 5, 4]
    s = LM.landmark_summary(table, ([5, 1, 3], [10.0, 4.0, 6.0, 5.0]), (0.5, 0.95))
    assert s['landmarks'] == 5 and s['empty_landmarks'] == 1 and s['landmarks_with_pit'] == 3
    assert s['of_mean_mean'] == 2.5 and s['of_mean_median'] == 2.5 and s['of_mean_max'] == 4.0
    assert s['sample_mean'] == 1.5 and s['sample_max'] == 5.0
    assert s['coverage'] == {'0.5': pytest.approx(1 / 3), '0.95': pytest.approx(2 / 3)}
    assert s['error_spread_correlation'] == pytest.approx(1.0)
    empty = LM.landmark_summary(np.full((2, 10), np.nan) * 0 + np.array([0] + [np.nan] * 9), ([2, 2, 0], [0.0, -math.inf, 0.0, -math.inf]), (0.5,))
    assert all(math.isnan(empty[k]) for k in ('of_mean_mean', 'of_mean_median', 'of_mean_max', 'sample_max', 'error_spread_correlation'))
    assert math.isnan(empty['coverage']['0.5'])


# ---------------------------------------------------------------- landmark files
def test_read_points_round_trip_comments_index_base_and_bad_lines(tmp_path):
    pts = np.array([[1.0, 2.5, 3.0], [10.0, 0.0, 7.25], [4.0, 4.0, 4.0]])
    path = tmp_path / 'fixed.txt'
    path.write_text('# three landmarks\n1 2.5 3\n\n10,0, 7.25   # trailing comment\n  4\t4  4\n')
    assert np.array_equal(LM.read_points(path), pts)
    assert np.array_equal(LM.read_points(str(path), index_base=1), pts - 1.0)
    np.savetxt(tmp_path / 'rt.txt', pts)
    assert np.array_equal(LM.read_points(tmp_path / 'rt.txt'), pts)
    for text, line in (('1 2 3\n4 5\n', 2), ('1 2 3\n\n# c\n1 2 x\n', 4), ('1 2 3 4\n', 1), ('1 2 nan\n', 1), ('1;2;3\n', 1)):
        bad = tmp_path / 'bad.txt'
        bad.write_text(text)
        with pytest.raises(ValueError, match=rf'bad\.txt, line {line}:'):
            LM.read_points(bad)
    (tmp_path / 'none.txt').write_text('# nothing\n\n')
    with pytest.raises(ValueError, match='no landmark'):
        LM.read_points(tmp_path / 'none.txt')
    with pytest.raises(ValueError, match='index_base'):
        LM.read_points(path, index_base=2)


def test_grid_points_follow_the_native_geometry():
    grid = NativeGrid.from_shape((7, 10, 13), (9, 9, 9), zooms=(2.0, 1.5, 1.0))
    assert grid.padding == (3, 1, 0) and grid.padded == (13, 12, 13)   # odd padding: the padded volume is no cube
    idx = np.array([[0, 0, 0], [6, 9, 12], [3, 4.5, 6], [2, 7, 11]], dtype=np.float64)
    got = LM.grid_points(idx, grid)
    for row, i in zip(got, idx):
        gc = grid.grid_coordinate(tuple(i))   # (D, H, W) order, registration-grid voxels
        want = [2.0 * gc[2] / 8 - 1.0, 2.0 * gc[1] / 8 - 1.0, 2.0 * gc[0] / 8 - 1.0]   # x, y, z
        assert row == pytest.approx(want, abs=1e-15)
    assert got[1] == pytest.approx([1.0, 2.0 * (10 / 11) - 1.0, 2.0 * (9 / 12) - 1.0])
    # positions in mm: normalised coordinates times mm_scale differ by the native index difference times the zoom
    mm = got * np.asarray(grid.mm_scale())
    assert (mm[1] - mm[0]) == pytest.approx([12 * 1.0, 9 * 1.5, 6 * 2.0])
    # without native volumes: indices of the registration grid itself
    reg = LM.registration_grid_points([[0, 0, 0], [4, 5, 6], [2, 2.5, 8]], (5, 6, 9))
    assert np.allclose(reg, [[-1, -1, -1], [0.5, 1.0, 1.0], [1.0, 0.0, 0.0]])
    assert (reg * np.asarray(DG.voxel_scale((5, 6, 9))))[1] == pytest.approx([6 - 4, 5 - 2.5, 4 - 2])


def test_synthetic_landmarks_are_the_blob_centres_of_the_generator():
    """The two landmark pairs reproduce synthetic_pair's images and sit on the maximum of each blob to the nearest voxel.  Each
    blob is looked at on its own: in the SUM the wide blob's slope pulls the narrow blob's peak to voxel (20, 13, 17) of the
    fixed image, 0.8 voxels from its centre (20.8, 12.8, 17.6), and leaves no second local maximum at all."""
    dims = (33, 33, 33)
    fixed_idx, moving_idx = synthetic.synthetic_landmarks(dims)
    assert fixed_idx.shape == moving_idx.shape == (2, 3)
    assert np.allclose(fixed_idx, [[16, 16, 16], [20.8, 12.8, 17.6]]) and np.allclose(moving_idx, [[17.28, 15.36, 16.8], [21.76, 13.6, 17.92]])
    f, m = synthetic.synthetic_pair(dims, noise=0)
    far = (100.0, 100.0, 100.0)   # a blob centred there is exactly 0 on the grid
    for im, blobs, idx in ((f['im'][0], synthetic.FIXED_BLOBS, fixed_idx), (m['im'][0], synthetic.MOVING_BLOBS, moving_idx)):
        shift_b = tuple(b - a for b, a in zip(blobs[1], synthetic.FIXED_BLOBS[1]))
        assert torch.equal(synthetic._blobs(dims, blobs[0], shift_b).float(), im)   # the constants ARE the generator's
        wide, narrow = synthetic._blobs(dims, blobs[0], far), synthetic._blobs(dims, far, shift_b)
        assert torch.equal((wide + narrow).float(), im)
        for blob, centre in ((wide, idx[0]), (narrow, idx[1])):
            peak = np.unravel_index(int(blob.argmax()), dims)
            assert peak == tuple(int(v) for v in np.rint(centre)), (peak, centre)
    # the same through the normalised coordinates the trainer uses: (z, y, x) of the issue -> (x, y, z) points
    pts = LM.registration_grid_points(fixed_idx, dims)
    assert np.allclose(pts, [[0, 0, 0], [0.1, -0.2, 0.3]])


# ---------------------------------------------------------------- the option parser
def _cfg(**landmarks):
    return {'log_period_MCMC': 5, 'no_samples_MCMC': 20, 'no_chains': 2, 'landmarks': landmarks}


class _Synthetic:
    native = None


class _Files:
    native = staticmethod(lambda: None)


def test_landmark_options(tmp_path):
    f, m = tmp_path / 'f.txt', tmp_path / 'm.txt'
    f.write_text('1 2 3\n4 5 6\n')
    m.write_text('2 3 4\n5 6 7\n')
    assert DG.landmark_options({'log_period_MCMC': 5, 'no_samples_MCMC': 20}) is None
    assert DG.landmark_options({**_cfg(), 'landmarks': False}) is None and DG.landmark_options({**_cfg(), 'landmarks': None}) is None
    o = DG.landmark_options(_cfg(fixed=str(f), moving=str(m), index_base=1))
    assert o['period'] == 5 and o['coverage_levels'] == (0.5, 0.95) and o['inverse'] is False and o['synthetic'] is False
    assert np.array_equal(o['fixed'], [[0, 1, 2], [3, 4, 5]]) and np.array_equal(o['moving'], [[1, 2, 3], [4, 5, 6]])
    o = DG.landmark_options(_cfg(synthetic=True, inverse=True, period=4, coverage_levels=[0.9]), _Synthetic())
    assert o == {'period': 4, 'index_base': 0, 'coverage_levels': (0.9,), 'inverse': True, 'synthetic': True, 'fixed': None, 'moving': None}
    names = DG.landmark_metric_names(o, 2)
    assert 'VI/train/TRE/median' in names and 'MCMC/chain_1/TRE_inverse/max' in names and 'MCMC/TRE/coverage_0.9' in names
    assert 'MCMC/TRE_inverse/error_spread_correlation' in names and len(names) == len(set(names)) == 3 + 2 * (4 + 5 + 1 + 1)
    both = dict(fixed=str(f), moving=str(m))
    m3 = tmp_path / 'm3.txt'
    m3.write_text('1 1 1\n')
    bad = tmp_path / 'bad.txt'
    bad.write_text('1 2\n')
    refusals = [
        ({'landmarks': True}, 'naming the two landmark files'),
        ({'landmarks': 'f.txt'}, 'must be true, false or'),
        (dict(both, colour=1), 'unknown keys'),
        (dict(both, period=0), 'period must be >= 1'),
        (dict(both, period=2.5), 'period must be an integer'),
        (dict(both, period=50), 'records no step'),
        (dict(fixed=str(f)), r'landmarks\.moving: the path'),
        (dict(moving=str(m)), r'landmarks\.fixed: the path'),
        (dict(fixed=str(f), moving=str(tmp_path / 'nowhere.txt')), 'cannot read'),
        (dict(fixed=str(f), moving=str(m3)), '2 fixed and 1 moving'),
        (dict(fixed=str(f), moving=str(bad)), r'bad\.txt, line 1'),
        (dict(both, index_base=2), 'index_base must be 0 or 1'),
        (dict(both, index_base=True), 'index_base must be 0 or 1'),
        (dict(both, inverse='yes'), 'inverse must be true or false'),
        (dict(synthetic=1), 'synthetic must be true or false'),
        (dict(both, synthetic=True), 'must not be given with it'),
        (dict(both, coverage_levels=[]), '1 to 8 coverage levels'),
        (dict(both, coverage_levels=[0.1] * 9), '1 to 8 coverage levels'),
        (dict(both, coverage_levels=[0.5, 1.0]), 'strictly increasing in'),
        (dict(both, coverage_levels=[0.0, 0.5]), 'strictly increasing in'),
        (dict(both, coverage_levels=[0.9, 0.5]), 'strictly increasing in'),
        (dict(both, coverage_levels=['a']), 'must be numbers'),
        (dict(both, coverage_levels=0.5), 'must be a list'),
    ]
    for opt, message in refusals:
        cfg = {**_cfg(), **opt} if 'landmarks' in opt else _cfg(**opt)
        with pytest.raises(ValueError, match=message):
            DG.landmark_options(cfg)
    with pytest.raises(ValueError, match='reads image files'):
        DG.landmark_options(_cfg(synthetic=True), _Files())
    with pytest.raises(ValueError, match='records; the record count holds'):
        DG.landmark_options({'log_period_MCMC': 1, 'no_samples_MCMC': 2 ** 30, 'no_chains': 4, 'landmarks': both})


def test_landmark_posterior_refuses_bad_geometry():
    for kw, message in ((dict(points=np.zeros((2, 3)), targets=np.zeros((3, 3))), 'both be'), (dict(points=np.zeros((0, 3)), targets=np.zeros((0, 3))), 'K >= 1'),
                        (dict(points=np.full((1, 3), np.nan), targets=np.zeros((1, 3))), 'finite'),
                        (dict(points=np.zeros((1, 3)), targets=np.zeros((1, 3)), scale=(1, 0, 1)), 'scale must hold'),
                        (dict(points=np.zeros((1, 3)), targets=np.zeros((1, 3)), dims=(1, 4, 4)), 'three dims')):
        with pytest.raises(ValueError, match=message):
            DG.LandmarkPosterior(**{'dims': (4, 4, 4), 'device': 'cpu', **kw})


# ---------------------------------------------------------------- the point-set writer
def test_write_vtk_points_matches_the_specification_fixture(tmp_path):
    points = [[1.5, -2.25, 0.125], [0, 10, -0.5], [33.75, 4, 1024]]
    scalars = [('tre_of_mean', [0.5, 1.25, 3]), ('std_major', [0.25, 0, 2.5]), ('pit', [0.75, float('nan'), 0.0625])]
    out = tmp_path / 'points.vtk'
    write_vtk_points(np.asarray(points), out, scalars, title='posterior-mean landmarks (mm)')
    want = open(os.path.join(ROOT, 'tests', 'golden', 'io', 'vtk_legacy_ascii_points.vtk'), 'rb').read()
    assert out.read_bytes() == want
    write_vtk_points(points, out, dict(scalars), title='posterior-mean landmarks (mm)')   # a dict of scalars, lists of points
    assert out.read_bytes() == want
    write_vtk_points([[0.1, 0.2, 0.3]], out)   # float32 values with nine significant digits, no POINT_DATA without scalars
    text = out.read_text().splitlines()
    assert text[4:] == ['POINTS 1 float', '0.100000001 0.200000003 0.300000012', 'VERTICES 1 2', '1 0']
    with pytest.raises(ValueError):
        write_vtk_points(np.zeros((2, 2)), out)
    with pytest.raises(ValueError):
        write_vtk_points(points, out, {'a b': [1, 2, 3]})
    with pytest.raises(ValueError):
        write_vtk_points(points, out, {'a': [1, 2]})


def test_save_landmarks_writes_the_table_and_the_points(tmp_path):
    import logging
    from ir_sgmcmc_amd.logger import save_landmarks
    from ir_sgmcmc_amd.ops import LANDMARK_COLUMNS
    assert tuple(LANDMARK_COLUMNS) == R.COLUMNS
    table = np.arange(20, dtype=np.float64).reshape(2, 10) / 4
    table[1, 9] = np.nan
    save_landmarks(logging.getLogger('test'), {'samples': tmp_path}, np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.5]]), table,
                   LANDMARK_COLUMNS, 'voxels', 'MCMC', '_inverse')
    rows = (tmp_path / 'MCMC_landmarks_inverse.csv').read_text().splitlines()
    assert rows[0] == 'landmark,mean_x,mean_y,mean_z,' + ','.join(R.COLUMNS) and len(rows) == 3
    assert rows[2].split(',')[:4] == ['1', '4.0', '5.0', '6.5'] and rows[2].split(',')[-1] == 'nan'
    assert [float(v) for v in rows[1].split(',')[4:]] == list(table[0])
    vtk = (tmp_path / 'MCMC_landmarks_inverse_mean.vtk').read_text().splitlines()
    assert vtk[1] == 'posterior-mean landmarks (voxels)' and vtk[4:7] == ['POINTS 2 float', '1 2 3', '4 5 6.5']
    assert vtk[vtk.index('SCALARS pit float 1') + 2:] == ['2.25', 'nan']
