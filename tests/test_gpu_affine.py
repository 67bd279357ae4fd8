"""The affine pre-alignment on the GPU: the operators of ir_sgmcmc_amd/affine.py against the numpy restatement of
tests/_affine.py (which shares no code with the HIP path), the refusals of their C ABI, the recovery of a known map, and the
trainer's `affine_init` option.

Sums: device and restatement form every TERM bit for bit alike (the documented order, every operation rounded once) and differ
only in the order of the sum.  A sum of N terms in any order is within (N - 1) 2^-53 sum|term| of the exact one (first order),
so |device - restatement| <= 2 (N - 1) 2^-53 sum|term| per column, sum|term| from the restatement.  On integer images under
integer maps every term is an integer far below 2^53 and the 94 values are EQUAL to the restatement's int64 ones.

Recovery: the device and the restatement run the same Levenberg-Marquardt loop on sums that differ by rounding only.  On an
MI355X their final maps were 3.0e-16 voxel (rigid, 24^3) and 2.7e-15 voxel (affine, 32^3) apart over the masked voxels, after the
same number of iterations; MAP_DISTANCE_BOUND is ten times the larger of the two (and far below the 1e-3 voxel it may never
exceed)."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import affine as A
from tests import _affine as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(9, 9, 9), (12, 13, 44), (5, 6, 70)]  # odd; no extent a multiple of the 64 x 4 block; a last axis longer than a wavefront


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def maps(shape):
    generic = (np.array([[1.03, 0.02, -0.01], [-0.015, 0.97, 0.025], [0.01, -0.02, 1.04]]), np.array([0.3, -0.45, 0.7]))
    return {'identity': (np.eye(3), np.zeros(3)),                      # every p on a node: the cell rule decides
            'shift_x_1': (np.eye(3), np.array([0.0, 0.0, 1.0])),        # integer p, the last column exactly at n - 1 or outside
            'generic': generic,
            'third_outside': (np.eye(3), np.array([0.0, 0.0, shape[2] / 3.0]))}   # the last third of the columns leaves


def volumes(shape, seed):
    rng = np.random.default_rng(seed)
    fixed, moving = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    return fixed, moving, rng.random(shape) < 0.7


def device_sums(fixed, moving, mask, lin, shift):
    """the 94 doubles as the device wrote them"""
    d = A.normal_equations(dev(fixed), dev(moving), None if mask is None else dev(mask), lin, shift)
    return np.concatenate([d['H'][np.triu_indices(12)], d['b'], [d['ssd'], d['n'], d['n_outside'], d['n_nonfinite']]]), d


def check_sums(name, got, want):
    n = want['terms']
    bound = 2.0 * max(n - 1, 0) * 2.0 ** -53 * want['abs'][:91]
    deviation = np.abs(got[:91] - want['sums'][:91])
    worst = int(np.argmax(deviation - bound))
    print(f'{name}: N = {n}, counts {got[91:].tolist()}, worst column {worst}: deviation {deviation[worst]:.3e}, bound {bound[worst]:.3e}')
    assert np.array_equal(got[91:], want['sums'][91:]), (name, got[91:], want['sums'][91:])
    assert np.isfinite(got).all() and (deviation <= bound).all(), (name, worst, deviation[worst], bound[worst])


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('which', ['identity', 'shift_x_1', 'generic', 'third_outside'])
@pytest.mark.parametrize('masked', [True, False])
def test_sums_against_the_restatement(shape, which, masked):
    fixed, moving, mask = volumes(shape, sum(shape))
    mask = mask if masked else None
    lin, shift = maps(shape)[which]
    got, d = device_sums(fixed, moving, mask, lin, shift)
    want = R.normal_equations(fixed, moving, mask, lin, shift)
    check_sums(f'{shape} {which} {"mask" if masked else "no mask"}', got, want)
    total = int(mask.sum()) if masked else int(np.prod(shape))
    assert d['n'] + d['n_outside'] + d['n_nonfinite'] == total and d['n'] > 0 and d['n_nonfinite'] == 0
    assert np.array_equal(d['H'], d['H'].T)
    if which == 'identity':
        assert d['n_outside'] == 0
    if which == 'shift_x_1':  # exactly the last column of the (masked) voxels leaves
        assert d['n_outside'] == (int(mask[:, :, -1].sum()) if masked else shape[0] * shape[1])
    if which == 'third_outside':  # x + W / 3 > W - 1: the last third of the columns, counted on the host
        gone = np.arange(shape[2]) + shape[2] / 3.0 > shape[2] - 1
        assert 0.3 < gone.mean() < 0.36
        assert d['n_outside'] == (int(mask[:, :, gone].sum()) if masked else shape[0] * shape[1] * int(gone.sum()))


def test_sums_with_non_finite_values():
    shape = (12, 13, 44)
    fixed, moving, mask = volumes(shape, 5)
    mask[3, 4, 5] = mask[6, 6, 20] = mask[6, 6, 21] = True
    fixed[3, 4, 5] = np.nan
    moving[6, 6, 21] = np.inf  # under the taps of up to eight cells
    fixed[0, 0, 43] = np.nan   # mapped outside by the shift below: counted as outside, whatever it holds
    mask[0, 0, 43] = True
    lin, shift = np.eye(3), np.array([0.25, 0.5, 0.75])
    got, d = device_sums(fixed, moving, mask, lin, shift)
    check_sums('non-finite', got, R.normal_equations(fixed, moving, mask, lin, shift))
    assert d['n_nonfinite'] >= 2 and d['n_outside'] > 0


@pytest.mark.parametrize('shift', [(0, 0, 0), (0, 0, 1), (1, -2, 0), (-3, 2, 4)])
def test_exact_case(shift):
    shape = (9, 9, 9)
    rng = np.random.default_rng(11)
    fixed, moving = rng.integers(-8, 9, shape).astype(np.float32), rng.integers(-8, 9, shape).astype(np.float32)
    mask = rng.random(shape) < 0.8
    for m in (mask, None):
        got, _ = device_sums(fixed, moving, m, np.eye(3), np.array(shift, dtype=np.float64))
        want = R.normal_equations(fixed, moving, m, np.eye(3, dtype=np.int64), np.array(shift), exact=True)['sums']
        assert want.dtype == np.int64 and np.abs(want).max() < 2 ** 53
        assert np.array_equal(got, want.astype(np.float64)), np.nonzero(got != want)[0]
        assert got[91] > 0


def test_determinism_and_the_empty_mask():
    shape = (12, 13, 44)
    fixed, moving, mask = volumes(shape, 3)
    lin, shift = maps(shape)['generic']
    a, _ = device_sums(fixed, moving, mask, lin, shift)
    b, _ = device_sums(fixed, moving, mask, lin, shift)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    empty, d = device_sums(fixed, moving, np.zeros(shape, bool), lin, shift)
    assert np.array_equal(empty, np.zeros(94)) and d['n'] == 0


# ---------------------------------------------------------------- the map as a tensor, and composed
TENSOR_SHAPES = [(3, 5, 70), (12, 13, 44), (2, 3, 2)]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize('shape', TENSOR_SHAPES)
@pytest.mark.parametrize('which', ['identity', 'generic'])
def test_affine_transformation_is_the_restatement_bit_for_bit(shape, which):
    lin, shift = maps(shape)[which]
    got = A.affine_transformation(lin, shift, shape, DEV).cpu().numpy()
    want = R.transformation(lin, shift, shape)
    assert got.shape == want.shape == (1, 3, *shape) and got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize('shape', TENSOR_SHAPES)
@pytest.mark.parametrize('Cn', [1, 2])
def test_compose_is_the_restatement_bit_for_bit(shape, Cn):
    lin, shift = maps(shape)['generic']
    rng = np.random.default_rng(Cn + sum(shape))
    phi = np.repeat(R.transformation(np.eye(3), np.zeros(3), shape), Cn, 0) + 0.05 * rng.standard_normal((Cn, 3, *shape)).astype(np.float32)
    total_t, total_d = A.compose(dev(phi), lin, shift)
    want_t, want_d = R.compose(phi, lin, shift)
    assert np.array_equal(bits(total_t.cpu().numpy()), bits(want_t)) and np.array_equal(bits(total_d.cpu().numpy()), bits(want_d))
    # composing the identity transformation with A gives A's own tensor, up to the float32 rounding of the identity grid
    ident = dev(np.repeat(R.transformation(np.eye(3), np.zeros(3), shape), Cn, 0))
    t, _ = A.compose(ident, lin, shift)
    assert float((t[:1] - A.affine_transformation(lin, shift, shape, DEV)).abs().max()) < 1e-5


def test_resampling():
    shape = (17, 17, 17)  # 16 intervals: the [-1, 1] coordinates of the nodes are dyadic and the warps hit them exactly
    rng = np.random.default_rng(2)
    moving = {'im': dev(rng.standard_normal((1, 1, *shape)).astype(np.float32)), 'mask': dev(rng.random((1, 1, *shape)) < 0.5),
              'seg': dev(rng.integers(0, 40, (1, 1, *shape)).astype(np.int16))}
    same = A.resample_pair(moving, np.eye(3), np.zeros(3))
    for k, v in moving.items():  # the identity gives the triple back bit for bit, as new tensors
        assert same[k].dtype == v.dtype and torch.equal(same[k], v) and same[k].data_ptr() != v.data_ptr()
    moved = A.resample_pair(moving, np.eye(3), np.array([0.0, 0.0, 1.0]))
    for k, v in moving.items():  # through the kernels: every voxel reads its right-hand neighbour, the last column itself (border)
        assert moved[k].dtype == v.dtype and moved[k].shape == v.shape
        assert torch.equal(moved[k][..., :-1], v[..., 1:]) and torch.equal(moved[k][..., -1], v[..., -1]), k
    ragged = (12, 13, 44)
    seg = dev(rng.integers(0, 40, (1, 1, *ragged)).astype(np.int16))
    out = A.resample_pair({'seg': seg}, np.eye(3), np.array([1.0, 0.0, -2.0]))['seg']  # nearest: exact at any extent
    assert torch.equal(out[:, :, :-1, :, 2:], seg[:, :, 1:, :, :-2])
    with pytest.raises(L.IrsError, match=r"moving\['im'\] must have shape \(1,1,D,H,W\)"):
        A.resample_pair({'im': moving['im'][0]}, np.eye(3), np.ones(3))


# ---------------------------------------------------------------- the C ABI refuses what it cannot do
def test_abi_refusals():
    lib = L.load()
    dims = (6, 6, 6)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    arr = lambda v: None if v is None else (C.c_double * len(v))(*v)
    eye, zero = [1.0, 0, 0, 0, 1, 0, 0, 0, 1], [0.0, 0, 0]
    im = torch.zeros(dims, device=DEV)
    sums = torch.full((L.IRS_AFFINE_SUMS,), 7.0, device=DEV, dtype=torch.float64)
    ws = torch.empty(L.IRS_AFFINE_WS_BYTES + 8, device=DEV, dtype=torch.uint8)
    out = torch.full((2, 3, *dims), 7.0, device=DEV)
    phi = torch.zeros(2, 3, *dims, device=DEV)

    def ne(f=im, m=im, d=dims, lin=eye, shift=zero, s=sums, w=ws, nbytes=L.IRS_AFFINE_WS_BYTES, offset=0):
        wp = None if w is None else C.c_void_p(w.data_ptr() + offset)
        return lib.irs_affine_normal_equations(p(f), p(m), None, *d, arr(lin), arr(shift), p(s), wp, nbytes, None)

    def tr(lin=eye, shift=zero, o=out, d=dims):
        return lib.irs_affine_transformation(arr(lin), arr(shift), p(o), *d, None)

    def co(t=phi, lin=eye, shift=zero, tt=out, td=None, Cn=2, d=dims):
        return lib.irs_affine_compose(p(t), arr(lin), arr(shift), p(tt), p(td), Cn, *d, None)

    bad_lin, bad_shift = eye[:4] + [float('nan')] + eye[5:], [0.0, float('inf'), 0.0]
    cases = [(lambda: ne(f=None), 'irs_affine_normal_equations: null pointer'),
             (lambda: ne(m=None), 'irs_affine_normal_equations: null pointer'),
             (lambda: ne(s=None), 'irs_affine_normal_equations: null pointer'),
             (lambda: ne(w=None), 'irs_affine_normal_equations: null pointer'),
             (lambda: ne(lin=None), 'irs_affine_normal_equations: null pointer'),
             (lambda: ne(shift=None), 'irs_affine_normal_equations: null pointer'),
             (lambda: ne(d=(6, 1, 6)), 'irs_affine_normal_equations: dims (6, 1, 6), every one >= 2 needed'),
             (lambda: ne(d=(1024, 1024, 1024)), 'irs_affine_normal_equations: the volume must have fewer than 2^30 voxels'),
             (lambda: ne(lin=bad_lin), 'irs_affine_normal_equations: lin[4] = nan is not finite'),
             (lambda: ne(shift=bad_shift), 'irs_affine_normal_equations: shift[1] = inf is not finite'),
             (lambda: ne(nbytes=L.IRS_AFFINE_WS_BYTES - 1),
              f'irs_affine_normal_equations: workspace of {L.IRS_AFFINE_WS_BYTES - 1} bytes, {L.IRS_AFFINE_WS_BYTES} needed (IRS_AFFINE_WS_BYTES)'),
             (lambda: ne(offset=4), 'irs_affine_normal_equations: the workspace must be 8-byte aligned'),
             (lambda: tr(o=None), 'irs_affine_transformation: null pointer'),
             (lambda: tr(lin=None), 'irs_affine_transformation: null pointer'),
             (lambda: tr(d=(6, 6, 1)), 'irs_affine_transformation: dims (6, 6, 1), every one >= 2 needed'),
             (lambda: tr(d=(70000, 2, 2)), 'irs_affine_transformation: 70000 planes are more than the 65535 rows of one launch'),
             (lambda: tr(shift=bad_shift), 'irs_affine_transformation: shift[1] = inf is not finite'),
             (lambda: co(t=None), 'irs_affine_compose: null pointer'),
             (lambda: co(tt=None, td=None), 'irs_affine_compose: total_transformation and total_displacement are both NULL, one is needed'),
             (lambda: co(Cn=0), f'irs_affine_compose: C = 0 chains, 1..{L.IRS_MAX_CHAINS}'),
             (lambda: co(Cn=L.IRS_MAX_CHAINS + 1), f'irs_affine_compose: C = {L.IRS_MAX_CHAINS + 1} chains, 1..{L.IRS_MAX_CHAINS}'),
             (lambda: co(shift=None), 'irs_affine_compose: null pointer'),
             (lambda: co(d=(0, 6, 6)), 'irs_affine_compose: dims (0, 6, 6), every one >= 2 needed'),
             (lambda: co(d=(40000, 2, 2)), 'irs_affine_compose: 80000 planes are more than the 65535 rows of one launch'),
             (lambda: co(lin=bad_lin), 'irs_affine_compose: lin[4] = nan is not finite')]
    for call, message in cases:
        assert call() != 0 and lib.irs_last_error().decode() == message, (lib.irs_last_error().decode(), message)
    torch.cuda.synchronize()
    assert (sums == 7.0).all() and (out == 7.0).all()  # nothing was launched
    assert ne() == 0 and co() == 0
    torch.cuda.synchronize()
    assert float(sums[91]) == 216.0 and float(sums[90]) == 0.0 and not (out == 7.0).any()
    with pytest.raises(L.IrsError, match='a map is lin'):
        A.normal_equations(im, im, None, np.eye(4), np.zeros(3))
    with pytest.raises(L.IrsError, match='moving shape'):
        A.normal_equations(im, torch.zeros(6, 6, 7, device=DEV), None, np.eye(3), np.zeros(3))


# ---------------------------------------------------------------- recovery of a known map
MAP_DISTANCE_BOUND = 2.8e-14  # voxel: ten times the measured 2.74e-15 (module docstring); never more than 1e-3


def cases():
    c, a = R.RIGID_CASE, R.affine_case()
    return {'rigid': (c['dims'], R.rodrigues(c['omega']), np.array(c['shift']), 'rigid', ()),
            'rigid_levels': (c['dims'], R.rodrigues(c['omega']), np.array(c['shift']), 'rigid', [[13, 13, 13]]),
            'affine': (a['dims'], a['lin'], a['shift'], 'affine', ())}


@pytest.mark.parametrize('name', ['rigid', 'rigid_levels', 'affine'])
def test_recovery(name):
    dims, lin, shift, kind, levels = cases()[name]
    fixed, moving, mask = R.analytic_pair(dims, lin, shift)
    t5 = lambda x: torch.from_numpy(x)[None, None]
    got_lin, got_shift, history = A.register(t5(fixed).to(DEV), t5(moving).to(DEV), t5(mask).to(DEV), A.AffineModel(kind), levels)
    error = R.map_error(got_lin, got_shift, lin, shift, mask)
    print(f'{name} {dims}: error {error:.4f} voxel (cap 0.1); {history}')
    assert [h['dims'] for h in history] == [tuple(lv) for lv in levels] + [dims]
    assert all(h['mean_ssd_last'] <= h['mean_ssd_first'] for h in history) and history[-1]['converged']
    assert error < 0.1
    if not levels:  # the same loop on the restatement
        ref_lin, ref_shift, ref_history = A.register(t5(fixed), t5(moving), t5(mask), A.AffineModel(kind), normal_eq=R.normal_eq_function)
        distance = R.map_error(got_lin, got_shift, ref_lin, ref_shift, mask)
        print(f'{name}: device and restatement maps {distance:.3e} voxel apart (bound {MAP_DISTANCE_BOUND:g}); iterations '
              f'{history[-1]["iterations"]} / {ref_history[-1]["iterations"]}')
        assert distance <= MAP_DISTANCE_BOUND


# ---------------------------------------------------------------- the trainer
N = 32
MISALIGN = {'rotation_deg': [4.0, 0.0, 0.0], 'shift': [0.0, 2.0, 0.0]}
KW = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4)


def make_trainer(tmp_path, affine_init, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128_affine.json')))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args'].update(dims=[N, N, N], misalign=MISALIGN)
    cfg['trainer'].update(**trainer_over)
    if affine_init is None:
        del cfg['trainer']['affine_init']
    else:
        cfg['trainer']['affine_init'] = affine_init
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, config.init_data_loader(), config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


def test_trainer_runs_the_pre_alignment(tmp_path):
    from ir_sgmcmc_amd.utils.imageio import read_vtk_vectors
    opt = {'model': 'rigid', 'levels': [[16, 16, 16]]}
    t = make_trainer(tmp_path / 'a', opt, **KW)
    t.run()
    s = t.affine_summary
    assert s['model'] == 'rigid' and [tuple(h['dims']) for h in s['history']] == [(16, 16, 16), (N, N, N)]
    assert s['SSD_after'] < s['SSD_before'] and 0.5 <= s['overlap'] <= 1.0 and s['iterations'] >= 2
    for key in ('lin', 'shift', 'index_matrix', 'normalised_matrix', 'mm_matrix'):
        assert np.isfinite(np.asarray(s[key])).all()
    metrics = t.metrics.result()
    for key in ('SSD_before', 'SSD_after', 'overlap', 'iterations'):
        assert metrics[f'affine/{key}'] == pytest.approx(s[key])
    # (the synthetic pair is one nearly round blob and a small one: the rotation about the line through the two is all but free,
    # so the map found is not compared with the loader's misalignment -- test_recovery does that on a pair that determines it)
    print(f'lin {s["lin"]}; shift {s["shift"]}; SSD {s["SSD_before"]:.5f} -> {s["SSD_after"]:.5f}; Dice {s["DSC_before"]} -> {s["DSC_after"]}')
    # Dice of the outer structure: before and after, and the step-0 metric sees the aligned pair
    outer = next(iter(t.structures_dict))
    assert s['DSC_after'][outer] > s['DSC_before'][outer]
    assert t.writer.scalars[f'VI/train/DSC/{outer}'][0] == 0
    # what was saved
    folder = t.config.save_dirs['samples']
    saved = json.load(open(folder / 'affine.json'))
    assert saved['lin'] == s['lin'] and saved['shift'] == s['shift'] and saved['model'] == 'rigid'
    assert (folder / 'MCMC_sample_mean_total.vtk').is_file()
    total = read_vtk_vectors(str(folder / 'MCMC_sample_mean_total.vtk'))[2]
    mean = read_vtk_vectors(str(folder / 'MCMC_sample_mean.vtk'))[2]
    from ir_sgmcmc_amd.utils import init_identity_grid_3D, transform_coordinates
    # the files hold float32 values in binary and the synthetic spacing is 1: compose of the saved mean is the saved total
    assert total.shape == mean.shape == (3, N, N, N) and np.array_equal(mean, t.displacement_mean.cpu().numpy())
    ident = init_identity_grid_3D((N, N, N), DEV).permute(0, 4, 1, 2, 3)
    _, want = A.compose((ident + transform_coordinates(dev(mean)[None])).contiguous(), s['lin'], s['shift'])
    assert np.array_equal(bits(total), bits(want[0].cpu().numpy()))
    assert float(np.abs(total - mean).max()) > 0.5  # the pre-alignment is in it: two voxels of shift and four degrees
    # a second run finds the same bits
    u = make_trainer(tmp_path / 'b', opt, **KW)
    u.run()
    assert u.affine_summary['lin'] == s['lin'] and u.affine_summary['shift'] == s['shift']


def test_trainer_without_the_option_and_the_refused_combinations(tmp_path):
    off = make_trainer(tmp_path / 'off', None, **KW)
    assert off.affine_options is None
    off.run()
    assert off.affine_summary is None and not any(k.startswith('affine/') for k in off.metrics.result())
    assert not (off.config.save_dirs['samples'] / 'affine.json').exists()
    with pytest.raises(ValueError, match='trainer.affine_init cannot be combined with trainer.landmarks'):
        make_trainer(tmp_path / 'l', {'model': 'rigid'}, landmarks={'synthetic': True}, **KW)
    with pytest.raises(ValueError, match='trainer.affine_init cannot be combined with trainer.native_resolution'):
        make_trainer(tmp_path / 'n', {'model': 'affine'}, native_resolution=True, **KW)
