"""Affine pre-alignment, the host side (no GPU): the trainer.affine_init refusals, the AffineModel Jacobian against central
differences, the round trips between index, normalised and mm matrices, carrying a map between levels, the synthetic loader's
misalignment, and the Levenberg-Marquardt loop of ir_sgmcmc_amd/affine.py run on the numpy restatement of tests/_affine.py
against an analytic truth.

The recovery cap of 0.1 voxel is a condition, not a measurement: it keeps the test from passing on a bad solver.  With this
loop the restatement reaches 0.021 voxel (rigid, 24^3) and 0.046 voxel (affine, 32^3)."""
import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import affine as A
from tests import _affine as R

FINE = (32, 32, 32)


def options(**affine_init):
    return {'affine_init': affine_init}


def test_the_option_is_off_when_absent():
    assert A.affine_init_options({}, FINE) is None
    assert A.affine_init_options({'affine_init': None}, FINE) is None
    assert A.affine_init_options({'affine_init': False}, FINE) is None


def test_the_option_fills_in_its_defaults():
    assert A.affine_init_options(options(model='rigid'), FINE) == {'model': 'rigid', 'levels': (), 'max_iters': 50, 'tol': 1e-3,
                                                                   'min_overlap': 0.5}
    got = A.affine_init_options(options(model='affine', levels=[[9, 10, 11], [16, 16, 16]], max_iters=7, tol=0.01, min_overlap=1), FINE)
    assert got == {'model': 'affine', 'levels': ((9, 10, 11), (16, 16, 16)), 'max_iters': 7, 'tol': 0.01, 'min_overlap': 1.0}


@pytest.mark.parametrize('cfg,message', [
    ({'affine_init': True}, 'trainer.affine_init must be {"model": "rigid" | "affine", ...}'),
    (options(model='rigid', lvls=[]), "trainer.affine_init: unknown keys ['lvls']"),
    (options(), "trainer.affine_init.model must be one of ['affine', 'rigid'], got None"),
    (options(model='similarity'), "trainer.affine_init.model must be one of ['affine', 'rigid'], got 'similarity'"),
    (options(model='rigid', max_iters=2.5), 'trainer.affine_init.max_iters must be an integer, got 2.5'),
    (options(model='rigid', max_iters=True), 'trainer.affine_init.max_iters must be an integer, got True'),
    (options(model='rigid', max_iters=0), 'trainer.affine_init: max_iters must be >= 1, got 0'),
    (options(model='rigid', tol=0), 'trainer.affine_init.tol must be a finite number > 0, got 0'),
    (options(model='rigid', tol='small'), "trainer.affine_init.tol must be a finite number > 0, got 'small'"),
    (options(model='rigid', min_overlap=0), 'trainer.affine_init.min_overlap must be a number in (0, 1], got 0'),
    (options(model='rigid', min_overlap=1.5), 'trainer.affine_init.min_overlap must be a number in (0, 1], got 1.5'),
    (options(model='rigid', levels=16), 'trainer.affine_init.levels must be a list of at most 4 levels [d, h, w], got 16'),
    (options(model='rigid', levels=[[9, 9, 9]] * 5), 'trainer.affine_init.levels must be a list of at most 4 levels'),
    (options(model='rigid', levels=[[16, 16]]), 'trainer.affine_init.levels[0] must be three integers [d, h, w], got [16, 16]'),
    (options(model='rigid', levels=[[16, 16, 16.0]]), 'trainer.affine_init.levels[0] must be three integers [d, h, w]'),
    (options(model='rigid', levels=[[8, 16, 16]]), 'trainer.affine_init.levels[0]: dims [8, 16, 16] have an extent below 9'),
    (options(model='rigid', levels=[[16, 16, 16], [12, 12, 12]]),
     'trainer.affine_init.levels[0]: dims [16, 16, 16] exceed [12, 12, 12] of levels[1]'),
    (options(model='rigid', levels=[[16, 33, 16]]), 'trainer.affine_init.levels[0]: dims [16, 33, 16] exceed [32, 32, 32] of the full grid'),
    (options(model='rigid', levels=[[32, 32, 32]]), 'trainer.affine_init.levels[0]: dims [32, 32, 32] are the full grid'),
    ({**options(model='rigid'), 'native_resolution': True},
     "trainer.affine_init cannot be combined with trainer.native_resolution: it addresses the moving image's own voxel space"),
    ({**options(model='affine'), 'landmarks': {'synthetic': True}},
     "trainer.affine_init cannot be combined with trainer.landmarks: it addresses the moving image's own voxel space"),
])
def test_option_refusals(cfg, message):
    with pytest.raises(ValueError) as e:
        A.affine_init_options(cfg, FINE)
    assert str(e.value).startswith(message), str(e.value)


def test_model_refusals():
    with pytest.raises(ValueError, match='an affine model is one of'):
        A.AffineModel('similarity')
    with pytest.raises(ValueError, match='spacing must hold three finite numbers > 0'):
        A.AffineModel('rigid', (1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match='a rigid map has 6 parameters'):
        A.AffineModel('rigid').matrix(np.zeros(12))


# ---------------------------------------------------------------- the model
SPACINGS = [(1.0, 1.0, 1.0), (2.5, 1.0, 0.8)]
THETAS = [np.zeros(6), np.array([1e-7, -2e-7, 1e-7, 0.5, 0.0, -1.0]), np.array([0.06, -0.05, 0.087, 1.5, -2.0, 1.0]),
          np.array([0.9, 1.4, -0.7, 0.0, 3.0, 0.0]), np.array([0.004, 0.003, -0.009, 0.0, 0.0, 0.0])]


def flat(model, theta):
    lin, shift = model.matrix(theta)
    return np.concatenate([lin.reshape(-1), shift])


@pytest.mark.parametrize('spacing', SPACINGS)
@pytest.mark.parametrize('theta', THETAS)
def test_rigid_jacobian_against_central_differences(spacing, theta):
    """float64 central differences with h = 1e-5: truncation h^2 |d3| / 6 ~ 2e-11 times the spacing ratio (<= 3.2), rounding
    2^-53 / h ~ 1e-11 -- the bound 1e-9 is a hundred times their sum"""
    model = A.AffineModel('rigid', spacing)
    P = model.jacobian(theta)
    assert P.shape == (12, 6)
    h = 1e-5
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        numeric = (flat(model, theta + e) - flat(model, theta - e)) / (2 * h)
        assert np.abs(P[:, i] - numeric).max() <= 1e-9, (i, np.abs(P[:, i] - numeric).max())


@pytest.mark.parametrize('spacing', SPACINGS)
def test_rigid_is_rigid_in_millimetres(spacing):
    model = A.AffineModel('rigid', spacing)
    lin, shift = model.matrix(THETAS[3])
    S = np.diag(spacing)
    Rm = S @ lin @ np.linalg.inv(S)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rm) - 1) < 1e-14
    assert np.array_equal(shift, THETAS[3][3:])
    assert np.abs(Rm - R.rodrigues(THETAS[3][:3])).max() < 1e-14  # against the restatement's own Rodrigues formula
    assert np.abs(model.from_map(lin, shift) - THETAS[3]).max() < 1e-12
    lin0, shift0 = model.matrix(model.identity())
    assert np.array_equal(lin0, np.eye(3)) and not shift0.any()


def test_affine_model_is_the_identity_parametrisation():
    model = A.AffineModel('affine')
    theta = np.arange(12.0)
    lin, shift = model.matrix(theta)
    assert np.array_equal(lin, theta[:9].reshape(3, 3)) and np.array_equal(shift, theta[9:])
    assert np.array_equal(model.jacobian(theta), np.eye(12)) and np.array_equal(model.from_map(lin, shift), theta)
    assert np.array_equal(flat(model, model.identity()), np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]))


# ---------------------------------------------------------------- matrices
def a_map():
    c = R.affine_case()
    return c['lin'], c['shift']


def test_matrix_round_trips():
    lin, shift = a_map()
    dims, spacing = (12, 13, 44), (2.5, 1.0, 0.8)
    for M, back in ((A.index_matrix(lin, shift, dims), lambda M: A.from_index_matrix(M, dims)),
                    (A.normalised_matrix(lin, shift, dims), lambda M: A.from_normalised_matrix(M, dims)),
                    (A.mm_matrix(lin, shift, dims, spacing), lambda M: A.from_mm_matrix(M, dims, spacing))):
        assert M.shape == (4, 4) and np.array_equal(M[3], [0, 0, 0, 1])
        l2, s2 = back(M)
        assert np.abs(l2 - lin).max() < 1e-14 and np.abs(s2 - shift).max() < 1e-13


def test_matrices_map_a_point_as_the_convention_says():
    lin, shift = a_map()
    dims, spacing = (12, 13, 44), np.array([2.5, 1.0, 0.8])
    c = (np.array(dims) - 1) / 2.0
    k = np.array([3.0, 7.5, 30.25])
    p = c + shift + lin @ (k - c)
    assert np.abs((A.index_matrix(lin, shift, dims) @ np.append(k, 1))[:3] - p).max() < 1e-12
    u = lambda x: 2 * x / (np.array(dims) - 1) - 1
    assert np.abs((A.normalised_matrix(lin, shift, dims) @ np.append(u(k), 1))[:3] - u(p)).max() < 1e-13
    assert np.abs((A.mm_matrix(lin, shift, dims, spacing) @ np.append(spacing * k, 1))[:3] - spacing * p).max() < 1e-12
    # the transformation tensor of the restatement is the normalised matrix applied to the identity grid
    t = R.transformation(lin, shift, dims)
    node = (5, 2, 17)
    want = (A.normalised_matrix(lin, shift, dims) @ np.append(u(np.array(node, float)), 1))[:3]
    assert np.abs(t[0, ::-1, node[0], node[1], node[2]] - want).max() < 1e-6


def test_carrying_a_map_between_levels():
    lin, shift = a_map()
    fine, coarse = (32, 33, 44), (9, 17, 12)
    l2, s2 = A.carry_map(lin, shift, fine, coarse)
    # the same physical map: a fine index K and its coarse coordinate k = rho K go to corresponding places
    rho = (np.array(coarse) - 1) / (np.array(fine) - 1)
    K = np.array([4.0, 20.0, 31.0])
    P = (A.index_matrix(lin, shift, fine) @ np.append(K, 1))[:3]
    p = (A.index_matrix(l2, s2, coarse) @ np.append(rho * K, 1))[:3]
    assert np.abs(p - rho * P).max() < 1e-12
    back = A.carry_map(l2, s2, coarse, fine)
    assert np.abs(back[0] - lin).max() < 1e-14 and np.abs(back[1] - shift).max() < 1e-14
    # a rigid map stays rigid, with the same rotation vector, in the coarser level's millimetres
    model = A.AffineModel('rigid', (2.5, 1.0, 0.8))
    theta = THETAS[2]
    level = model.at_level(fine, coarse)
    assert np.allclose(level.spacing * rho, model.spacing, rtol=1e-15)
    got = level.from_map(*A.carry_map(*model.matrix(theta), fine, coarse))
    assert np.abs(got[:3] - theta[:3]).max() < 1e-12 and np.abs(got[3:] - rho * theta[3:]).max() < 1e-12


def test_corners_and_their_motion():
    mask = np.zeros((9, 10, 11), bool)
    mask[2:5, 3:9, 1:4] = True
    corners = A.box_corners(mask, mask.shape)
    assert corners.shape == (8, 3) and sorted(map(tuple, corners))[0] == (2, 3, 1) and sorted(map(tuple, corners))[-1] == (4, 8, 3)
    assert sorted(map(tuple, A.box_corners(None, (9, 10, 11))))[-1] == (8, 9, 10)
    ident = (np.eye(3), np.zeros(3))
    assert A.corner_motion(ident, (np.eye(3), np.array([0.0, 3.0, 4.0])), corners, mask.shape) == 5.0


# ---------------------------------------------------------------- the synthetic loader's misalignment
def test_the_synthetic_pair_is_unchanged_by_default_and_misaligned_on_request():
    from ir_sgmcmc_amd.data_loader import SyntheticDataLoader, synthetic_pair
    f0, m0 = synthetic_pair((17, 17, 17), seed=3)
    f1, m1 = synthetic_pair((17, 17, 17), seed=3, misalign=None)
    assert all(torch.equal(f0[k], f1[k]) and torch.equal(m0[k], m1[k]) for k in f0)
    f2, m2 = synthetic_pair((17, 17, 17), seed=3, misalign={'rotation_deg': [0, 0, 0], 'shift': [0, 0, 2]})
    assert all(torch.equal(f0[k], f2[k]) for k in f0)
    for k in m0:  # moved by two voxels along x; 17 nodes: the [-1, 1] grid of the host warp is dyadic, so the nodes are hit exactly
        assert m2[k].dtype == m0[k].dtype and m2[k].shape == m0[k].shape
        assert torch.equal(m2[k][..., :-2], m0[k][..., 2:]), k
    _, m3 = synthetic_pair((17, 17, 17), seed=3, misalign={'rotation_deg': [4, 0, 0], 'shift': [0, 2, 0]})
    assert not torch.equal(m3['im'], m0['im']) and m3['seg'].dtype == torch.int16 and m3['mask'].dtype == torch.bool
    with pytest.raises(ValueError, match='misalign: unknown keys'):
        synthetic_pair((17, 17, 17), misalign={'angle': 3})
    plain, moved = SyntheticDataLoader((17, 17, 17), seed=3), SyntheticDataLoader((17, 17, 17), seed=3, misalign={'shift': [0, 0, 2]})
    assert torch.equal(next(iter(plain))[1]['im'][0], m0['im']) and torch.equal(next(iter(moved))[1]['im'][0], m2['im'])


# ---------------------------------------------------------------- the solver on the restatement
def recover(dims, lin, shift, kind):
    fixed, moving, mask = R.analytic_pair(dims, lin, shift)
    t5 = lambda x: torch.from_numpy(x)[None, None]
    got_lin, got_shift, history = A.register(t5(fixed), t5(moving), t5(mask), A.AffineModel(kind), normal_eq=R.normal_eq_function)
    return R.map_error(got_lin, got_shift, lin, shift, mask), history


def test_rigid_recovery_on_the_restatement():
    c = R.RIGID_CASE
    error, history = recover(c['dims'], R.rodrigues(c['omega']), np.array(c['shift']), 'rigid')
    h = history[-1]
    print(f'rigid {c["dims"]}: error {error:.4f} voxel (cap 0.1), {h}')
    assert len(history) == 1 and h['converged'] and h['accepted'] >= 1 and h['mean_ssd_last'] < h['mean_ssd_first']
    assert h['overlap'] >= 0.5 and h['dims'] == c['dims']
    assert error < 0.1


def test_affine_recovery_on_the_restatement():
    c = R.affine_case()
    error, history = recover(c['dims'], c['lin'], c['shift'], 'affine')
    h = history[-1]
    print(f'affine {c["dims"]}: error {error:.4f} voxel (cap 0.1), {h}')
    assert h['converged'] and h['mean_ssd_last'] < h['mean_ssd_first']
    assert error < 0.1


def test_the_loop_rejects_a_step_that_loses_the_overlap_and_a_start_without_any():
    c = R.RIGID_CASE
    fixed, moving, mask = R.analytic_pair(c['dims'], R.rodrigues(c['omega']), np.array(c['shift']))
    model = A.AffineModel('rigid')
    ne = lambda lin, shift: R.normal_eq_function(fixed, moving, mask, lin, shift)
    corners, n = A.box_corners(mask, c['dims']), int(mask.sum())
    with pytest.raises(ValueError, match='the start map leaves 0 of'):
        A.levenberg_marquardt(ne, model, np.array([0, 0, 0, 100.0, 0, 0]), corners, c['dims'], n)
    # with min_overlap = 1 every voxel must stay inside: steps that push one out are rejected, and what is accepted keeps n
    theta, hist = A.levenberg_marquardt(ne, model, model.identity(), corners, c['dims'], n, min_overlap=1.0)
    assert ne(*model.matrix(theta))['n'] == n and hist['overlap'] == 1.0
    # one trial step and no more
    _, hist = A.levenberg_marquardt(ne, model, model.identity(), corners, c['dims'], n, max_iters=1)
    assert hist['iterations'] == 1 and not hist['converged']


def test_unpacking_the_sums():
    v = np.arange(94.0)
    d = A.unpack_sums(v)
    mine = R.as_dict(v)
    assert np.array_equal(d['H'], mine['H']) and np.array_equal(d['H'], d['H'].T) and d['H'][0, 11] == 11 and d['H'][1, 1] == 12
    assert np.array_equal(d['b'], np.arange(78.0, 90.0)) and (d['ssd'], d['n'], d['n_outside'], d['n_nonfinite']) == (90.0, 91, 92, 93)
