"""Landmark propagation on the GPU: ops.transform_points bit for bit on the exact cases and within the derived per-element
bound of tests/_landmarks.py on smooth fields, the clamp and the NaN rows, the recorder against the float64 reference, the
inverse direction against the inverse-consistency error the project measures for the same field, the trainer option and the
error paths."""
import copy
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import ops as G
from ir_sgmcmc_amd.diagnostics import LandmarkPosterior, landmark_metric_names, voxel_scale
from tests import _landmarks as R
from tests._exact_cases import EXACT_DIMS
from tests._report import check

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = R.U


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous()


def first_mismatch(a, b):
    idx = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
    return f'{len(idx)} elements differ, first at {idx[0].tolist()}: {a[tuple(idx[0])]!r} != {b[tuple(idx[0])]!r}'


# ---------------------------------------------------------------- bit for bit
@pytest.mark.parametrize('dims', EXACT_DIMS)
def test_exact_cases_bit_for_bit(dims):
    """tests/test_landmarks_host.py proves that float32 and float64 agree bit for bit on these inputs, so the kernel is held to
    equality with the float64 reference cast to float32: a difference is an indexing, clamp, weight or order error"""
    pts, field, scale, offset = R.exact_case(dims)
    s64 = R.sample(pts, field, np.float64)
    m64 = R.mapped(s64, scale, offset, np.float64)
    mapped, sampled = G.transform_points(dev(pts), dev(field), scale, dev(offset), want_sampled=True)
    mapped, sampled = mapped.cpu().numpy(), sampled.cpu().numpy()
    assert sampled.shape == mapped.shape == (3, len(pts), 3) and sampled.dtype == np.float32
    assert np.array_equal(sampled, s64.astype(np.float32)), f'{dims} sampled: ' + first_mismatch(sampled, s64.astype(np.float32))
    assert np.array_equal(mapped, m64.astype(np.float32)), f'{dims} mapped: ' + first_mismatch(mapped, m64.astype(np.float32))
    # mapped alone (sampled NULL), without an offset and with the unit scale: the sampled values themselves
    alone = G.transform_points(dev(pts), dev(field)).cpu().numpy()
    assert np.array_equal(alone, (s64 + 0.0).astype(np.float32))


def test_translation_maps_every_point_by_the_vector():
    dims, vec = (5, 6, 7), (0.75, -1.5, 2.25)
    field = np.broadcast_to(np.asarray(vec, dtype=np.float32).reshape(1, 3, 1, 1, 1), (2, 3, *dims)).copy()
    pts = R.random_points(129, 5, reach=0.999)
    for scale in ((1.0, 1.0, 1.0), (2.0, 0.5, 4.0)):
        mapped, sampled = G.transform_points(dev(pts), dev(field), scale, want_sampled=True)
        # the weights of a point are exact and sum to 1, but their eight products with the constant are rounded: 10 u |v|
        assert float((sampled.cpu() - torch.tensor(vec)).abs().max()) <= R.sample_bound(field)
        want = torch.tensor([s * v for s, v in zip(scale, vec)])
        assert float((mapped.cpu() - want).abs().max()) <= max(scale) * R.sample_bound(field) + U * float(want.abs().max())
    # dyadic positions: exactly the vector, and exactly scale * vector + offset
    cells = np.stack([np.arange(0, n - 0.75, 0.25)[:17] * (2.0 / (n - 1)) - 1.0 for n in (9, 9, 9)], axis=1).astype(np.float32)
    f9 = np.broadcast_to(np.asarray(vec, dtype=np.float32).reshape(1, 3, 1, 1, 1), (1, 3, 9, 9, 9)).copy()
    mapped = G.transform_points(dev(cells), dev(f9), (2.0, 0.5, 4.0), dev(np.full_like(cells, 8.0))).cpu()
    assert torch.equal(mapped, torch.tensor([[8 + 1.5, 8 - 0.75, 8 + 9.0]]).expand(1, 17, 3))


def test_points_outside_the_box_take_the_border_values_and_nonfinite_points_give_nan_rows():
    dims = (5, 6, 7)
    field = R.smooth_field(2, dims, 77)
    D, H, W = dims
    corners = [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    pts = np.asarray([tuple(1.5 * c for c in p) for p in corners] + [tuple(float(c) for c in p) for p in corners], dtype=np.float32)
    sampled = G.transform_points(dev(pts), dev(field), want_sampled=True)[1].cpu().numpy()
    for k, (sx, sy, sz) in enumerate(corners + corners):
        want = field[:, :, (D - 1) * (sz > 0), (H - 1) * (sy > 0), (W - 1) * (sx > 0)]
        assert np.array_equal(sampled[:, k], want), (k, sampled[:, k], want)
    # one axis outside: the clamp of that axis, the others interpolate as the point on the face does
    inside = R.random_points(33, 78, reach=0.9)
    out, face = inside.copy(), inside.copy()
    out[:, 0], face[:, 0] = 1.5, 1.0
    out[::2, 2], face[::2, 2] = -1.5, -1.0
    a, b = (G.transform_points(dev(p), dev(field)).cpu() for p in (out, face))
    assert torch.equal(a, b)
    # NaN and +-inf coordinates: NaN rows in both outputs, the other rows untouched
    base = R.random_points(70, 79)
    bad = base.copy()
    bad[3, 1], bad[7, 0], bad[64, 2], bad[69] = np.nan, np.inf, -np.inf, np.nan
    off = dev(np.ones_like(base))
    m0, s0 = G.transform_points(dev(base), dev(field), (2.0, 2.0, 2.0), off, want_sampled=True)
    m1, s1 = G.transform_points(dev(bad), dev(field), (2.0, 2.0, 2.0), off, want_sampled=True)
    rows = torch.tensor([k in (3, 7, 64, 69) for k in range(70)])
    for good, got in ((m0, m1), (s0, s1)):
        good, got = good.cpu(), got.cpu()
        assert bool(torch.isnan(got[:, rows]).all()) and torch.equal(got[:, ~rows], good[:, ~rows]) and bool(torch.isfinite(good).all())


# ---------------------------------------------------------------- smooth fields within the derived bound
WORST = {}


@pytest.mark.parametrize('K', R.SMOOTH_K)
@pytest.mark.parametrize('C', R.SMOOTH_CHAINS)
@pytest.mark.parametrize('dims', R.SMOOTH_DIMS)
def test_smooth_fields_within_the_derived_bound(dims, C, K):
    """every element within u (10 max|d| + 6 (n_max - 1) L) of the float64 reference (tests/_landmarks.py derives it,
    tests/test_landmarks_host.py shows that a float32 evaluation reaches an eighth of it)"""
    pts, field, offset = R.smooth_case(dims, C, K)
    s64 = R.sample(pts, field, np.float64)
    m64 = R.mapped(s64, R.SMOOTH_SCALE, offset, np.float64)
    mapped, sampled = G.transform_points(dev(pts), dev(field), R.SMOOTH_SCALE, dev(offset), want_sampled=True)
    assert sampled.shape == (C, K, 3)
    bound = R.sample_bound(field)
    err = check('landmarks_smooth', f'sampled {dims}', sampled.cpu(), torch.from_numpy(s64), bound)
    WORST['sampled'] = max(WORST.get('sampled', 0.0), err / bound)
    print(f'sampled {dims} C={C} K={K}: max error {err:.3e}, bound {bound:.3e} (worst so far {WORST["sampled"]:.3f} of the bound)')
    merr = (mapped.cpu().double() - torch.from_numpy(m64)).abs().amax(dim=(0, 1)).numpy()
    mb = R.mapped_bound(field, R.SMOOTH_SCALE, offset, m64)
    print(f'mapped: max error per channel {merr}, bound {mb}')
    assert (merr <= mb).all()
    # the float32 restatement in the kernel's rounding order: the kernel IS that arithmetic
    s32 = R.sample(pts, field, np.float32)
    assert np.array_equal(sampled.cpu().numpy(), s32), first_mismatch(sampled.cpu().numpy(), s32)


def test_large_point_sets_use_the_grid_stride_loop():
    """C K beyond the 4096 x 256 threads of the launch: the same rows as in small calls"""
    dims, Kbig = (5, 6, 7), 4096 * 256 // 2 + 3
    field = dev(R.smooth_field(3, dims, 91))
    pts = dev(R.random_points(Kbig, 92))
    big = G.transform_points(pts, field)
    for lo in (0, Kbig // 2 - 5, Kbig - 300):
        assert torch.equal(big[:, lo:lo + 300], G.transform_points(pts[lo:lo + 300].contiguous(), field))


# ---------------------------------------------------------------- the recorder
def _posterior(pts, targets):
    return LandmarkPosterior(pts, targets, R.RECORDER_DIMS, DEV)


def _run_records(lp, fields, poison=None):
    records = []
    for s, f in enumerate(fields):
        f = f.copy()
        if poison is not None and s == poison[0]:
            f[poison[1], :, 0:2, 0:2, 0:2] = np.nan   # the eight voxels around landmark 0, and around no other landmark
        lp.record(dev(f))
        records.append(lp.last_mapped.cpu().numpy())
    return records


def test_recorder_against_the_float64_reference():
    pts, targets, fields = R.recorder_case()
    lp = _posterior(pts, targets)
    records = _run_records(lp, fields, poison=(2, 1))
    assert lp.records == R.RECORDER_STEPS * R.RECORDER_CHAINS == 10 and records[0].shape == (2, R.RECORDER_K, 3)
    # the mapped points are the operator's: the displacement in voxels on top of the landmark's own position in voxels
    vs = np.asarray(voxel_scale(R.RECORDER_DIMS))
    want = R.mapped(R.sample(pts.astype(np.float32), fields[0], np.float32), (1.0, 1.0, 1.0), (pts * vs).astype(np.float32), np.float32)
    assert np.array_equal(records[0], want)
    nan_rows = np.isnan(records[2]).any(axis=2)
    assert nan_rows[1, 0] and nan_rows.sum() == 1   # landmark 0 of chain 1 in the third record, nothing else
    target = lp.target.cpu().numpy()
    samples = R.update(records, target)
    ref, bounds = R.finalize(samples, target), R.state_bounds(samples, target)
    state = {k: v.cpu().numpy() for k, v in lp.state.items()}
    counts = np.full(R.RECORDER_K, 10)
    counts[0] = 9
    assert np.array_equal(state['count'], counts) and state['count'].dtype == np.int32
    for key, per in (('mean', 'mean'), ('comoment', 'comoment'), ('tre_mean', 'tre_mean'), ('tre_m2', 'tre_m2')):
        got, want = state[key], (ref[key] if key in ref else ref['table'][:, 1])
        tol = bounds[per] if got.ndim == 1 else bounds[per][:, None]
        err = np.abs(got - want)
        print(f'{key}: worst error {err.max():.3e}, worst error / bound {(err / tol).max():.3f}')
        assert (err <= tol).all(), key
    assert (np.abs(state['tre_max'] - ref['table'][:, 3]) <= bounds['tre_mean']).all()
    table, summary = lp.finalize((0.5, 0.95))
    tol = R.table_bounds(ref, bounds)
    assert np.array_equal(table[:, 0], counts) and np.isfinite(table).all() and np.isfinite(tol).all()
    err = np.abs(table - ref['table'])
    for j, name in enumerate(R.COLUMNS):
        print(f'{name}: worst error {err[:, j].max():.3e}, worst error / bound {(err[:, j] / np.maximum(tol[:, j], 1e-300)).max():.3f}')
    assert (err <= tol).all(), [(R.COLUMNS[j], k) for k, j in np.argwhere(err > tol)]
    assert (np.diff(table[:, 5:8], axis=1) <= 0).all() and (table[:, 9] >= 0).all() and (table[:, 9] <= 1).all()
    print('pit:', np.sort(table[:, 9])[[0, 16, 32, 48, 64]])
    # the summary: the device's fixed-order sums against sums of the reference table
    _, isum, fsum = G.landmark_finalize(lp.state, lp.target)
    assert isum.tolist() == ref['isummary'] == [R.RECORDER_K, 0, R.RECORDER_K]
    fsum, K = fsum.tolist(), R.RECORDER_K
    assert abs(fsum[0] - ref['fsummary'][0]) <= tol[:, 4].sum() + K * 2.0 ** -53 * ref['fsummary'][0]
    assert abs(fsum[1] - ref['fsummary'][1]) <= tol[:, 4].max()
    assert abs(fsum[2] - ref['fsummary'][2]) <= tol[:, 1].sum() + K * 2.0 ** -53 * ref['fsummary'][2]
    assert abs(fsum[3] - ref['fsummary'][3]) <= tol[:, 3].max()
    assert summary['records'] == 10 and summary['landmarks'] == K and summary['empty_landmarks'] == 0
    assert summary['of_mean_mean'] == fsum[0] / K and summary['of_mean_max'] == fsum[1] and summary['sample_max'] == fsum[3]
    assert summary['of_mean_median'] == float(np.median(table[:, 4]))
    assert summary['coverage'] == {'0.5': float((table[:, 9] <= 0.5).mean()), '0.95': float((table[:, 9] <= 0.95).mean())}
    assert summary['error_spread_correlation'] == pytest.approx(np.corrcoef(table[:, 4], table[:, 5])[0, 1], abs=1e-12)
    # last_tre: the record just taken
    mean, peak = lp.last_tre()
    e = np.sqrt(((records[-1].astype(np.float64) - target.astype(np.float64)) ** 2).sum(axis=2))
    assert mean == pytest.approx(e.mean(axis=1), rel=1e-12) and peak == pytest.approx(e.max(axis=1), rel=1e-12)
    # 3 + 2 records across state_dict / load_state_dict: bit-identical
    first = _posterior(pts, targets)
    for s, f in enumerate(fields[:3]):
        g = f.copy()
        if s == 2:
            g[1, :, 0:2, 0:2, 0:2] = np.nan
        first.record(dev(g))
    sd = copy.deepcopy(first.state_dict())
    second = _posterior(pts, targets)
    second.load_state_dict(sd)
    assert second.records == 6
    for f in fields[3:]:
        second.record(dev(f))
    assert second.records == 10
    for k in lp.state:
        assert torch.equal(second.state[k], lp.state[k]), k
    with pytest.raises(ValueError, match='not those of this run'):
        _posterior(pts[::-1].copy(), targets).load_state_dict(sd)


def test_fewer_than_four_records_and_zero_spread_give_nan_pit():
    pts, targets, fields = R.recorder_case()
    three = LandmarkPosterior(pts, targets, R.RECORDER_DIMS, DEV)
    three.record(dev(np.concatenate([fields[0], fields[1][:1]])))   # one step of C = 3 chains
    table, summary = three.finalize()
    assert (table[:, 0] == 3).all() and np.isnan(table[:, 8:]).all() and np.isfinite(table[:, :8]).all()
    assert summary['landmarks_with_pit'] == 0 and summary['empty_landmarks'] == 0 and math.isnan(summary['coverage']['0.5'])
    # a landmark never seen: a NaN target position cannot be built through the class, so through the operator
    mapped = torch.full((2, 4, 3), float('nan'), device=DEV)
    mapped[:, 1:] = torch.arange(18, device=DEV, dtype=torch.float32).reshape(2, 3, 3)
    target = torch.zeros(4, 3, device=DEV)
    state = G.landmark_state(4, DEV)
    for k in range(3):
        G.landmark_update(mapped + k * (mapped % 5), target, state, 2 * k)
    t, isum, fsum = (x.cpu() for x in G.landmark_finalize(state, target))
    assert t[:, 0].tolist() == [0, 6, 6, 6] and bool(torch.isnan(t[0, 1:]).all()) and bool(torch.isfinite(t[1:, :8]).all())
    assert isum.tolist() == [4, 1, int(torch.isfinite(t[:, 9]).sum())]
    assert fsum[1].item() == t[1:, 4].max().item() and fsum[3].item() == t[1:, 3].max().item()
    # the same sample every time: no spread, principal stds exactly 0, pit NaN and not inf
    same = LandmarkPosterior(pts, targets, R.RECORDER_DIMS, DEV)
    field = dev(np.repeat(fields[0][:1], 2, axis=0))
    for _ in range(3):
        same.record(field)
    table, summary = same.finalize()
    assert (table[:, 0] == 6).all() and (table[:, 5:8] == 0).all() and (table[:, 2] == 0).all()
    assert np.isnan(table[:, 8:]).all() and summary['landmarks_with_pit'] == 0
    assert np.array_equal(table[:, 1], table[:, 3]) and np.allclose(table[:, 1], table[:, 4], rtol=1e-14)


# ---------------------------------------------------------------- the inverse direction
def test_forward_then_inverse_returns_within_the_inverse_consistency_error():
    """A fixed point x is carried to y = x + d(x) by exp(v) and back to y + d_inv(y) by exp(-v).  At a voxel centre that is the
    residual ops.inverse_consistency measures, r(x) = d(x) + trilinear(d_inv)(x + d(x)), so the point returns to within the
    norm of r at its voxel plus what float32 adds on the way (all in voxels, per component, then sqrt(3) for the norm):
      E1    the forward position: the sampler's bound on d, and the product and the sum of mapped = d * (2 / (n - 1)) + x on
            values of at most 1.1 normalised units, 2 * 1.1 u (n_max - 1) / 2 voxels; the operator's own t(x) carries as much;
      d_inv sampled at a position off by 2 E1 along each axis: 3 L_inv * 2 E1, plus the sampler's bound on d_inv;
      E3    the product and the sum of the way back, as in E1; u max|d| for the rounded sum inside r itself.
    Off the voxel centres the same round trip is held to its float64 evaluation on the same fields."""
    dims, no_steps = (10, 14, 22), 12
    v = dev(R.smooth_field(2, dims, 311, amplitude=1.0))
    t, d, _ = G.svf_exp_fwd(v, no_steps)
    t_inv, d_inv = G.svf_exp_inverse(v, no_steps)
    norm, _, _, fsum = G.inverse_consistency(t, d, d_inv)
    vs = np.asarray(voxel_scale(dims))
    to_norm = tuple(1.0 / s for s in vs)
    D, H, W = dims
    z, y, x = np.meshgrid(np.arange(1, D - 1), np.arange(1, H - 1), np.arange(1, W - 1), indexing='ij')
    pick = np.random.default_rng(3).choice(z.size, 257, replace=False)
    idx = np.stack([x.ravel()[pick], y.ravel()[pick], z.ravel()[pick]], axis=1)
    centres = (idx / vs - 1.0).astype(np.float32)
    d_h, dinv_h = d.cpu().numpy(), d_inv.cpu().numpy()
    round_1 = 2 * 1.1 * U * (max(dims) - 1) / 2
    E1 = R.sample_bound(d_h) + round_1
    L_inv = R.adjacent_difference(dinv_h)
    # (and the norm map itself is a float32 root of float32 squares: 4 u of its value)
    extra = math.sqrt(3.0) * (2 * E1 * (1 + 3 * L_inv) + R.sample_bound(dinv_h) + round_1 + U * float(np.abs(d_h).max()))

    def round_trip(points):
        fwd = G.transform_points(dev(points), d, to_norm, dev(points))            # (C,K,3) normalised positions in the moving space
        back = torch.stack([G.transform_points(fwd[c].contiguous(), d_inv[c:c + 1].contiguous(), to_norm, fwd[c].contiguous())[0]
                            for c in range(fwd.shape[0])])
        return fwd, back

    fwd, back = round_trip(centres)
    err = ((back.cpu().double() - torch.from_numpy(centres).double()) * torch.from_numpy(vs)).norm(dim=2).numpy()   # (C,K) voxels
    ice = norm.cpu().numpy()[:, 0, idx[:, 2], idx[:, 1], idx[:, 0]].astype(np.float64)
    moved = ((fwd.cpu().double() - torch.from_numpy(centres).double()) * torch.from_numpy(vs)).norm(dim=2)
    print(f'round trip at voxel centres: worst {err.max():.3e} voxels, inverse-consistency error there up to {ice.max():.3e} '
          f'(field max {fsum[:, 2].max().item():.3e}), float32 allowance {extra:.3e}; the points moved up to {float(moved.max()):.3f} voxels')
    assert float(moved.max()) > 0.25 and (err <= ice * (1 + 4 * U) + extra).all(), float((err - ice).max())
    # off the grid: against the float64 evaluation of the same round trip on the same fields
    pts = R.random_points(257, 4, reach=0.8)
    fwd, back = round_trip(pts)
    fwd64 = R.mapped(R.sample(pts, d_h, np.float64), to_norm, pts, np.float64)
    back64 = np.stack([R.mapped(R.sample(fwd64[c].astype(np.float32), dinv_h[c:c + 1], np.float64), to_norm, fwd64[c].astype(np.float32),
                                np.float64)[0] for c in range(2)])
    # fwd64 enters the way back rounded to float32 (one more rounding of a position, inside round_1 taken twice)
    tol = math.sqrt(3.0) * ((E1 + round_1) * (1 + 3 * L_inv) + R.sample_bound(dinv_h) + round_1)
    off = ((back.cpu().double().numpy() - back64) * vs)
    print(f'round trip off the grid against float64: worst {np.abs(off).max():.3e} voxels, allowance {tol:.3e}')
    assert np.sqrt((off ** 2).sum(axis=2)).max() <= tol


# ---------------------------------------------------------------- the trainer
def make_trainer(tmp_path, dims=24, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128.json')))
    cfg['trainer'].update(save_dir=str(tmp_path), **trainer_over)
    cfg['data_loader']['args']['dims'] = [dims] * 3
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, config.init_data_loader(), config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


KW = dict(no_chains=2, no_iters_burn_in=30, no_samples_MCMC=30, log_period_MCMC=10)


def test_trainer_logs_the_target_registration_error(tmp_path):
    n = 24
    torch.manual_seed(0)
    on = make_trainer(tmp_path / 'on', n, landmarks={'synthetic': True, 'inverse': True}, **KW)
    on.run()
    res = on.metrics.result()
    names = landmark_metric_names(on.landmark_options, 2)
    assert all(on.metrics._count[k] > 0 and math.isfinite(res[k]) for k in names if 'correlation' not in k and 'coverage' not in k), \
        [k for k in names if not on.metrics._count.get(k)]
    for key in ['VI/train/TRE/mean', 'VI/train/TRE/median', 'VI/train/TRE/max', 'MCMC/chain_0/TRE/mean', 'MCMC/chain_1/TRE/max',
                'MCMC/chain_1/TRE_inverse/mean', 'MCMC/chain_0/TRE_inverse/max', 'MCMC/TRE/of_mean_mean', 'MCMC/TRE/of_mean_median',
                'MCMC/TRE/of_mean_max', 'MCMC/TRE/sample_mean', 'MCMC/TRE/sample_max', 'MCMC/TRE/coverage_0.5', 'MCMC/TRE/coverage_0.95',
                'MCMC/TRE/error_spread_correlation', 'MCMC/TRE_inverse/of_mean_mean', 'MCMC/TRE_inverse/coverage_0.95']:
        assert key in names and on.metrics._count[key] > 0, key
    assert on.metrics._count['MCMC/chain_0/TRE/mean'] == 3 and on.metrics._count['VI/train/TRE/mean'] == 1
    # step 0: the analytic distance of the two pairs in voxels, from the generator's shifts (z, y, x) in [-1,1] units.  The
    # positions are float32 values of at most (n - 1) / 2 voxels: two roundings per component of a difference
    shifts = np.asarray([(0.08, -0.04, 0.05), (0.06, 0.05, 0.02)])
    initial = np.sqrt(((shifts * (n - 1) / 2) ** 2).sum(axis=1))
    tol = math.sqrt(3.0) * 2 * U * (n - 1) / 2
    assert abs(res['VI/train/TRE/mean'] - initial.mean()) <= tol and abs(res['VI/train/TRE/max'] - initial.max()) <= tol
    assert abs(res['VI/train/TRE/median'] - np.median(initial)) <= tol
    # registration reduces the landmark error
    print(f'TRE of the unregistered pair {res["VI/train/TRE/mean"]:.4f} voxels, of the posterior mean {res["MCMC/TRE/of_mean_mean"]:.4f}, '
          f'inverse {res["MCMC/TRE_inverse/of_mean_mean"]:.4f}')
    assert res['MCMC/TRE/of_mean_mean'] < res['VI/train/TRE/mean']
    s = on.landmark_summary
    assert s['unit'] == 'voxels' and set(s) == {'unit', 'TRE', 'TRE_inverse'}
    assert s['TRE']['records'] == 6 and s['TRE']['landmarks'] == 2 and len(s['TRE']['table']) == 2 and len(s['TRE']['table'][0]) == 10
    assert s['TRE']['of_mean_mean'] == res['MCMC/TRE/of_mean_mean'] and s['TRE']['columns'] == list(G.LANDMARK_COLUMNS)
    folder = on.config.save_dirs['samples']
    for tag in ('', '_inverse'):
        rows = open(os.path.join(str(folder), f'MCMC_landmarks{tag}.csv')).read().splitlines()
        assert len(rows) == 3 and rows[0].startswith('landmark,mean_x,mean_y,mean_z,count,tre_mean')
        vtk = open(os.path.join(str(folder), f'MCMC_landmarks{tag}_mean.vtk')).read().splitlines()
        assert vtk[2:5] == ['ASCII', 'DATASET POLYDATA', 'POINTS 2 float'] and 'SCALARS tre_of_mean float 1' in vtk
    assert float(rows[1].split(',')[4]) == 6.0
    # the checkpoint key exists with the option only
    assert set(on.state_dict()['landmarks']) == {'TRE', 'TRE_inverse'}
    # with the option absent: the same chain, no TRE key, no landmark file, every other metric bit-identical
    torch.manual_seed(0)
    off = make_trainer(tmp_path / 'off', n, **KW)
    off.run()
    assert torch.equal(off.v_curr_state.view(torch.int32), on.v_curr_state.view(torch.int32))
    off_res = off.metrics.result()
    assert not any('TRE' in k for k in off_res) and [k for k in res if 'TRE' not in k] == list(off_res)
    assert sorted(res) == sorted(list(off_res) + names)
    for k, value in off_res.items():
        assert value == res[k] or (math.isnan(value) and math.isnan(res[k])), k
    assert not [f for f in os.listdir(str(off.config.save_dirs['samples'])) if 'landmarks' in f]
    assert off.landmark_options is None and off.landmark_summary is None and 'landmarks' not in off.state_dict()


def test_trainer_reads_landmark_files_and_resumes(tmp_path):
    """the two files instead of "synthetic", forward only, and a run resumed from a checkpoint ends in the same table"""
    n = 16
    from ir_sgmcmc_amd.data_loader import synthetic_landmarks
    fixed_idx, moving_idx = synthetic_landmarks((n, n, n))
    np.savetxt(tmp_path / 'fixed.txt', fixed_idx + 1, header='counted from 1')
    np.savetxt(tmp_path / 'moving.txt', moving_idx + 1, delimiter=',')
    opt = {'fixed': str(tmp_path / 'fixed.txt'), 'moving': str(tmp_path / 'moving.txt'), 'index_base': 1, 'period': 4, 'coverage_levels': [0.9]}
    kw = dict(no_chains=2, no_iters_burn_in=4, no_samples_MCMC=16, log_period_MCMC=8, save_outputs=False)
    torch.manual_seed(0)
    whole = make_trainer(tmp_path / 'whole', n, landmarks=opt, checkpoint_period=12, **kw)
    whole.run()
    assert whole.landmark_summary['TRE']['records'] == 8 and 'TRE_inverse' not in whole.landmark_summary
    assert 'MCMC/TRE/coverage_0.9' in whole.metrics.result() and whole.metrics._count['MCMC/chain_1/TRE/max'] == 4
    ckpt = whole.config.save_dirs['checkpoints'] / 'checkpoint_0000012.pt'
    assert 'landmarks' in torch.load(ckpt, map_location='cpu', weights_only=True)
    torch.manual_seed(0)
    resumed = make_trainer(tmp_path / 'resumed', n, landmarks=opt, resume=str(ckpt), **kw)
    resumed.run()
    assert json.dumps(resumed.landmark_summary, sort_keys=True) == json.dumps(whole.landmark_summary, sort_keys=True)


# ---------------------------------------------------------------- error paths
def test_error_paths():
    field = dev(R.smooth_field(2, (5, 6, 7), 1))
    pts = dev(R.random_points(9, 2))
    for call, message in (
            (lambda: G.transform_points(pts, field[:, :2].contiguous()), r'\(C,3,D,H,W\)'),
            (lambda: G.transform_points(pts[:, :2].contiguous(), field), r'points must be a \(K,3\)'),
            (lambda: G.transform_points(pts.double(), field), 'torch.float64'),
            (lambda: G.transform_points(pts[:0], field), 'K = 0 points'),
            (lambda: G.transform_points(pts, field, offset=pts[:5].contiguous()), r'offset must be a \(9,3\)'),
            (lambda: G.transform_points(pts.cpu(), field), 'CPU tensor'),
            (lambda: G.transform_points(pts, field.cpu()), 'CPU tensor'),
            (lambda: G.transform_points(pts, field, (1.0, 0.0, 1.0)), 'finite floats > 0'),
            (lambda: G.transform_points(pts, field, (1.0, -2.0, 1.0)), 'finite floats > 0'),
            (lambda: G.transform_points(pts, field, (1.0, float('inf'), 1.0)), 'finite floats > 0'),
            (lambda: G.landmark_update(torch.zeros(2, 9, 3, device=DEV), pts[:5].contiguous(), G.landmark_state(9, DEV), 0), r'target must be a \(9,3\)'),
            (lambda: G.landmark_update(torch.zeros(2, 9, 3, device=DEV), pts, G.landmark_state(8, DEV), 0), r'mean must be a \(9, 3\)'),
            (lambda: G.landmark_update(torch.zeros(2, 9, 3, device=DEV), pts, G.landmark_state(9, 'cpu'), 0), 'CPU tensor'),
            (lambda: G.landmark_update(torch.zeros(2, 9, 3, device=DEV), pts, G.landmark_state(9, DEV), -1), 'records_before'),
            (lambda: G.landmark_update(torch.zeros(9, 9, 3, device=DEV), pts, G.landmark_state(9, DEV), 0), 'C = 9 chains'),
            (lambda: G.landmark_finalize({**G.landmark_state(9, DEV), 'count': torch.zeros(9, device=DEV)}, pts), 'count must be'),
    ):
        with pytest.raises(L.IrsError, match=message):
            call()
    # through the library itself: both outputs NULL, K out of range, a bad scale, bad dims, NULL inputs
    lib = L.load()
    out = torch.empty(2, 9, 3, device=DEV)
    p, f, o, st = L.dev_ptr(pts), L.dev_ptr(field), L.dev_ptr(out), L.stream_ptr()
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    for args, message in (((p, 9, f, 2, 5, 6, 7, one, None, None, None, st), 'no output requested'),
                          ((p, 0, f, 2, 5, 6, 7, one, None, None, o, st), 'K = 0'),
                          ((p, (1 << 24) + 1, f, 2, 5, 6, 7, one, None, None, o, st), 'K = 16777217'),
                          ((p, 9, f, 9, 5, 6, 7, one, None, None, o, st), 'C = 9 chains'),
                          ((p, 9, f, 2, 1, 6, 7, one, None, None, o, st), 'bad dims'),
                          ((p, 9, f, 2, 5, 6, 7, (C.c_float * 3)(1.0, 0.0, 1.0), None, None, o, st), 'scale[1] = 0'),
                          ((p, 9, f, 2, 5, 6, 7, (C.c_float * 3)(float('nan'), 1.0, 1.0), None, None, o, st), 'scale[0] = nan'),
                          ((None, 9, f, 2, 5, 6, 7, one, None, None, o, st), 'bad arguments'),
                          ((p, 9, f, 2, 5, 6, 7, None, None, None, o, st), 'bad arguments')):
        assert lib.irs_transform_points(*args) != 0
        assert message in lib.irs_last_error().decode(), (message, lib.irs_last_error())
    state = [L.dev_ptr(t) for t in G.landmark_state(9, DEV).values()]
    table, isum, fsum = torch.empty(9, 10, device=DEV, dtype=torch.float64), torch.empty(3, device=DEV, dtype=torch.int64), \
        torch.empty(4, device=DEV, dtype=torch.float64)
    ws = torch.empty(L.IRS_LANDMARK_WS_BYTES, device=DEV, dtype=torch.uint8)
    assert lib.irs_landmark_finalize(*state, p, 9, L.dev_ptr(table), L.dev_ptr(isum), L.dev_ptr(fsum), L.dev_ptr(ws),
                                     L.IRS_LANDMARK_WS_BYTES - 1, st) != 0 and b'IRS_LANDMARK_WS_BYTES' in lib.irs_last_error()
    assert lib.irs_landmark_finalize(*state, p, 9, None, L.dev_ptr(isum), L.dev_ptr(fsum), L.dev_ptr(ws), L.IRS_LANDMARK_WS_BYTES, st) != 0
    assert lib.irs_landmark_update(o, p, 2, 9, *state[:5], None, 0, st) != 0 and b'bad arguments' in lib.irs_last_error()
    torch.cuda.synchronize()
