"""Posterior principal modes without a GPU ("Displacement modes"): the host algebra of modes.modes_decompose
on a hand-checked case, against an SVD of the data matrix and against centring the data; the option parsing; the split-R-hat of
the scores; and the bounds of tests/_displacement_modes.py held by numpy evaluations of the very inputs the GPU tests use."""
import math

import numpy as np
import pytest

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.diagnostics import (MODES_METRICS, displacement_modes_options, modes_summary, voxel_scale)
from ir_sgmcmc_amd.modes import modes_decompose
from tests import _displacement_modes as R


def test_hand_checked_case():
    """2 x 2 x 3 grid, four records +-a psi_1, +-b psi_2 with psi_1, psi_2 orthonormal over the mask, scale 1: lambda =
    (2 a^2 / 3, 2 b^2 / 3, 0), shares a^2 / (a^2 + b^2) and b^2 / (a^2 + b^2), modes along psi_1 and psi_2"""
    shape, a, b = (2, 2, 3), 3.0, 1.5
    V = 12
    mask = np.ones(shape, dtype=bool)
    mask[0, 0, 0] = False
    psi1, psi2 = np.zeros((3, V)), np.zeros((3, V))
    psi1[0, 1:5] = 0.5                      # four voxels of channel 0
    psi2[1, 5:9] = 0.5                      # four voxels of channel 1, one of them negative (every value exact in float32)
    psi2[1, 5] *= -1
    records = np.stack([a * psi1, -a * psi1, b * psi2, -b * psi2]).reshape((4, 3) + shape).astype(np.float32)
    G3 = R.gram_np(records, mask)
    dec = modes_decompose(G3, (1.0, 1.0, 1.0), int(mask.sum()), [0, 0, 0, 0], 8)
    assert np.allclose(dec['eigenvalues'], [2 * a * a / 3, 2 * b * b / 3, 0.0], rtol=1e-14, atol=1e-15)
    assert np.allclose(dec['explained'][:2], [a * a / (a * a + b * b), b * b / (a * a + b * b)], rtol=1e-14)
    assert dec['n90'] == 2 and dec['scores'].shape == (4, 3) and dec['coeff'].shape == (3, 4)
    assert math.isclose(dec['var_total'], 2 * (a * a + b * b) / 3, rel_tol=1e-14)
    assert math.isclose(dec['participation'], (a * a + b * b) ** 2 / (a ** 4 + b ** 4), rel_tol=1e-13)
    assert np.allclose(dec['std'][:2], np.sqrt(np.array([2 * a * a / 3, 2 * b * b / 3]) / 11), rtol=1e-14)
    assert np.isnan(dec['rhat']).all()      # one chain
    # the sign rule on the eigenvectors: the entry of largest magnitude positive, the lowest index on the tie +-1/sqrt 2
    e = dec['eigenvectors']
    assert np.allclose(e[:, 0], [math.sqrt(0.5), -math.sqrt(0.5), 0, 0], atol=1e-15)
    assert np.allclose(e[:, 1], [0, 0, math.sqrt(0.5), -math.sqrt(0.5)], atol=1e-15)
    out = R.project_np(records, dec['coeff'][:2], (1.0, 1.0, 1.0))
    fields = out['a'].reshape(2, 3, V)
    assert np.allclose(fields[0], math.sqrt(2 * a * a / 3) * psi1, atol=1e-15)
    assert np.allclose(fields[1], math.sqrt(2 * b * b / 3) * psi2, atol=1e-15)
    moved = (records.reshape(4, 3, V) != 0).any(axis=(0, 1)).reshape(shape)
    assert np.allclose(out['explained'][moved], 1.0, atol=2e-7) and not out['explained'][~moved].any()
    assert not out['mean'].any()
    # scores: sqrt((n - 1) lambda) e
    assert np.allclose(dec['scores'][:, 0], [a, -a, 0, 0], atol=1e-14) and np.allclose(dec['scores'][:, 1], [0, 0, b, -b], atol=1e-14)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('n', [2, 5, 12])
def test_against_an_svd_of_the_data_matrix(n, masked):
    shape = (5, 6, 7)
    mask = R.make_mask('random', shape) if masked else None
    records = R.random_records(n, shape, 40 + n)
    scale = voxel_scale(shape)
    k = int(np.prod(shape)) if mask is None else int(mask.sum())
    dec = modes_decompose(R.gram_np(records, mask), scale, k, None, 16)
    lam, fields, Xc = R.svd_np(records, scale, mask)
    K = min(16, n - 1)
    assert np.allclose(dec['eigenvalues'], lam[:n - 1], rtol=1e-12, atol=1e-14 * lam[0])
    got = dec['coeff'] @ R.data_matrix(records, scale, mask)     # the mode fields, masked and scaled
    for m in range(K):
        sign = 1.0 if got[m] @ fields[m] > 0 else -1.0
        assert np.allclose(got[m], sign * fields[m], rtol=0, atol=1e-9 * math.sqrt(lam[0]))
        assert math.isclose(np.linalg.norm(got[m]), math.sqrt(dec['eigenvalues'][m]), rel_tol=1e-10)
    # the restatement agrees with the package
    lam2, U2, _ = R.decompose_np(R.gram_np(records, mask), scale, k)
    assert np.array_equal(lam2, dec['eigenvalues']) and np.array_equal(U2[:, :K], dec['eigenvectors'])
    assert dec['n'] == n and math.isclose(dec['var_total'], (Xc ** 2).sum() / (n - 1), rel_tol=1e-12)


@pytest.mark.parametrize('n,Cn', R.PLANTED_CASES)
def test_centring_in_gram_space_against_centring_the_data(n, Cn):
    shape = (16, 12, 20)
    records, psi, scale = R.planted_records(n, shape, 100 * n + Cn)
    _, _, Gc = R.decompose_np(R.gram_np(records), scale, int(np.prod(shape)))
    X = R.data_matrix(records, scale)
    Xc = X - X.mean(axis=0, keepdims=True)
    lam1 = np.linalg.eigvalsh(Xc @ Xc.T / (n - 1)).max()
    err = np.abs(Gc - Xc @ Xc.T / (n - 1)).max()
    print({'centring: worst entry error / lambda_1': err / lam1})
    assert err <= 2e-15 * lam1
    lam = np.sort(np.linalg.eigvalsh(Gc))[::-1]
    assert ((lam[:3] - lam[1:4]) / lam[:3] >= 0.5).all()


def test_one_record_and_bad_shapes():
    dec = modes_decompose(np.ones((3, 1, 1)), (1, 1, 1), 5, [0], 4)
    assert dec['n'] == 1 and dec['eigenvalues'].size == 0 and dec['coeff'].shape == (0, 1) and dec['var_total'] == 0.0
    for bad in (np.zeros((2, 3, 3)), np.zeros((3, 2, 3)), np.zeros((3, 0, 0))):
        with pytest.raises(ValueError):
            modes_decompose(bad, (1, 1, 1), 5)


def base(**over):
    return {'no_samples_MCMC': 100, 'log_period_MCMC': 10, 'no_chains': 2, **over}


def test_option_parsing():
    assert displacement_modes_options(base()) is None
    for off in (False, None):
        assert displacement_modes_options(base(displacement_modes=off)) is None
    assert displacement_modes_options(base(displacement_modes=True)) == {'period': 10, 'modes': 8, 'max_records': 256, 'save': True}
    assert displacement_modes_options(base(displacement_modes={'period': 5, 'modes': 16, 'max_records': 40, 'save': False})) == \
        {'period': 5, 'modes': 16, 'max_records': 40, 'save': False}
    assert displacement_modes_options(base(displacement_modes={'max_records': 1024}))['max_records'] == L.IRS_MODES_MAX_RECORDS
    assert displacement_modes_options(base(displacement_modes={'max_records': 20}))['max_records'] == 20  # exactly the ceiling
    refusals = (
        (dict(displacement_modes='yes'), 'must be true, false or'),
        (dict(displacement_modes={'modes': 3, 'bins': 4}), "unknown keys ['bins']"),
        (dict(displacement_modes={'period': 2.5}), 'period must be an integer'),
        (dict(displacement_modes={'period': True}), 'period must be an integer'),
        (dict(displacement_modes={'period': 0}), 'the period must be >= 1'),
        (dict(displacement_modes={'period': 101}), 'records no step'),
        (dict(displacement_modes={'modes': 0}), 'modes must be in 1 .. 16, got 0'),
        (dict(displacement_modes={'modes': 17}), 'modes must be in 1 .. 16, got 17'),
        (dict(displacement_modes={'modes': 2.0}), 'modes must be an integer'),
        (dict(displacement_modes={'modes': True}), 'modes must be an integer'),
        (dict(displacement_modes={'max_records': 1}), 'max_records must be in 2 .. 1024, got 1'),
        (dict(displacement_modes={'max_records': 1025}), 'max_records must be in 2 .. 1024, got 1025'),
        (dict(displacement_modes={'max_records': '64'}), 'max_records must be an integer'),
        (dict(displacement_modes={'save': 1}), 'save must be true or false'),
        (dict(displacement_modes={'max_records': 19}), '10 steps of 2 chains are 20 records; the store holds at most 19'),
        (dict(displacement_modes=True, no_samples_MCMC=3000), 'the store holds at most 256'),
        (dict(displacement_modes={'period': 100}, no_chains=1), 'modes need at least 2'),
    )
    for over, text in refusals:
        with pytest.raises(ValueError) as e:
            displacement_modes_options(base(**over))
        assert text in str(e.value), (over, str(e.value))
        assert str(e.value).startswith('trainer.displacement_modes')
    assert MODES_METRICS == ('var_total', 'explained_1', 'explained_M', 'n90', 'participation', 'std_1', 'rhat_max')


def test_metric_names_follow_the_covariance_keys():
    import copy
    import json
    import os
    from ir_sgmcmc_amd.parse_config import ConfigParser
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = json.load(open(os.path.join(root, 'configs', 'synthetic_ssd_l2_128_modes.json')))
    names = ConfigParser.from_dict(copy.deepcopy(cfg), make_dirs=False).init_metrics()
    i = names.index('MCMC/modes/var_total')
    assert names[i - 1].startswith('MCMC/covariance/') and names[i:i + 7] == [f'MCMC/modes/{k}' for k in MODES_METRICS]
    cfg['trainer'].pop('displacement_modes')
    assert not [k for k in ConfigParser.from_dict(copy.deepcopy(cfg), make_dirs=False).init_metrics() if 'modes' in k]


def test_split_rhat_of_the_scores():
    """the scalar formula on the host against the restatement of ops.split_rhat's, and against a direct evaluation"""
    rng = np.random.default_rng(5)
    n, Cn = 24, 3
    records, _, scale = R.planted_records(n, (5, 6, 7), 9)
    chain = list(range(Cn)) * (n // Cn)
    dec = modes_decompose(R.gram_np(records), scale, 210, chain, 3)
    for m in range(3):
        series = np.stack([dec['scores'][np.asarray(chain) == c, m] for c in range(Cn)])
        assert math.isclose(dec['rhat'][m], R.split_rhat_np(series), rel_tol=1e-14)
        h = series.shape[1] // 2
        seqs = [s[:h] for s in series] + [s[-h:] for s in series]
        Wv = np.mean([np.var(s, ddof=1) for s in seqs])
        Bn = np.var([np.mean(s) for s in seqs], ddof=1)
        assert math.isclose(dec['rhat'][m], math.sqrt(((h - 1) / h * Wv + Bn) / Wv), rel_tol=1e-12)
    s = modes_summary(dec, 3)
    assert s['rhat_max'] == np.nanmax(dec['rhat']) and s['modes'] == 3 and s['records'] == n
    # fewer than four records per chain, or one chain: NaN
    assert np.isnan(modes_decompose(R.gram_np(records[:9]), scale, 210, chain[:9], 3)['rhat']).all()
    assert np.isnan(modes_decompose(R.gram_np(records), scale, 210, [0] * n, 3)['rhat']).all()
    assert R.split_rhat_np(np.ones((2, 8))) == 1.0 and R.split_rhat_np(np.array([[1.0] * 8, [2.0] * 8])) == math.inf
    del rng


@pytest.mark.parametrize('index', range(len(R.GRAM_CASES)))
def test_gram_bound_holds_for_a_float64_numpy_evaluation(index):
    """the very inputs of the GPU test: numpy's float64 sums (pairwise, another order than the kernel's) stay within gamma_k
    sum |x_i x_j| of math.fsum, and are exact on the dyadic family"""
    records, mask, ref, bound = R.gram_case(index, 'random')
    G = R.gram_np(records, mask)
    assert (np.abs(G - ref) <= bound).all()
    # a float32 evaluation is NOT within it (the bound is tight enough to tell the precisions apart) wherever there is a sum
    if bound.max() > 0 and (mask is None or mask.sum() > 8):
        x = records.reshape(records.shape[0], 3, -1)
        x = x if mask is None else x[:, :, mask.reshape(-1)]
        G32 = np.einsum('icv,jcv->cij', x, x).astype(np.float64)
        assert (np.abs(G32 - ref) > bound).any()
    records, mask, ref, bound = R.gram_case(index, 'dyadic')
    assert not bound.any() and np.array_equal(R.gram_np(records, mask), ref)
    exact = np.rint(ref * 256)
    assert np.array_equal(exact / 256, ref)  # integers over 2^8: nothing was rounded


@pytest.mark.parametrize('n,M,recipe', R.PROJECT_CASES)
@pytest.mark.parametrize('shape', R.SHAPES[:3])
def test_explained_bound_holds_for_the_restatement(shape, n, M, recipe):
    """the float64 restatement in the kernel's order against the centred float64 reference, on the GPU test's inputs"""
    records, coeff, scale, out, ref = R.project_case(shape, n, M, recipe)
    R.check_explained(out['explained'], ref)
    assert out['mean'].dtype == np.float32 and out['modes'].shape == (M, 3) + shape
    if n == 1:
        assert not out['explained'].any() and np.array_equal(out['mean'], records[0])
