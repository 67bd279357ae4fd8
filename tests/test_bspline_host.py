"""Cubic B-spline output resampling on the host: the option, and the restatement of tests/_bspline.py against scipy and
against itself (node reproduction).  No GPU."""
import numpy as np
import pytest

from ir_sgmcmc_amd import bspline
from tests import _bspline as B

SHAPES = [(2, 3, 70), (5, 6, 7), (9, 9, 9), (12, 13, 44), (2, 2, 2)]


def volume(shape, seed=0):
    return np.random.default_rng(seed).random(shape).astype(np.float32)


# ---------------------------------------------------------------- the option
@pytest.mark.parametrize('cfg', [{}, {'output_interpolation': None}, {'output_interpolation': 'linear'}])
def test_option_off(cfg):
    assert bspline.output_interpolation_options(cfg) is None


def test_option_cubic():
    assert bspline.output_interpolation_options({'output_interpolation': 'cubic'}) == {'order': 3}


@pytest.mark.parametrize('value', ['Cubic', 'nearest', 'quadratic', '', 3, 1, True, False, ['cubic'], {'order': 3}, 3.0])
def test_option_refusals(value):
    with pytest.raises(ValueError, match='"linear" or "cubic"'):
        bspline.output_interpolation_options({'output_interpolation': value})


# ---------------------------------------------------------------- against scipy
@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_against_scipy(shape):
    """the recursion with an all-float64 store against spline_filter, and its float64 evaluation against map_coordinates
    (order 3, mode 'mirror'), both within 2^-40 max|c|: three double recursions, 64 products."""
    ndimage = pytest.importorskip('scipy.ndimage')
    s = volume(shape).astype(np.float64)
    c = B.prefilter(s, store=np.float64)
    ref = ndimage.spline_filter(s, order=3, mode='mirror', output=np.float64)
    bound = 2.0 ** -40 * np.abs(ref).max()
    err = np.abs(c - ref).max()
    print(f'{shape}: max|c| {np.abs(ref).max():.4g}, coefficients {err:.3g}, bound {bound:.3g}')
    assert c.dtype == np.float64 and err <= bound
    rng = np.random.default_rng(1)
    q = [rng.random(500) * (n - 1) for n in shape]
    for a, n in enumerate(shape):  # the ends and a few nodes among them
        q[a][:4] = [0.0, n - 1.0, 1.0, n - 2.0]
    value = B.evaluate(c, tuple(q), np.float64)
    ref_value = ndimage.map_coordinates(s, np.stack(q), order=3, mode='mirror', output=np.float64)
    err = np.abs(value - ref_value).max()
    print(f'{shape}: values {err:.3g}')
    assert err <= bound


# ---------------------------------------------------------------- node reproduction
@pytest.mark.parametrize('shape', SHAPES)
def test_nodes_come_back(shape):
    """float32 store, float32 evaluation at the identity: the image within 70 * 2^-24 max|c| (64 products and the weights)"""
    s = volume(shape, seed=2)
    c = B.prefilter(s)
    assert c.dtype == np.float32
    q = tuple(g.astype(np.float32) for g in np.meshgrid(*[np.arange(n) for n in shape], indexing='ij'))
    back = B.evaluate(c, q)
    bound = 70 * 2.0 ** -24 * np.abs(c).max()
    err = np.abs(back.astype(np.float64) - s).max()
    print(f'{shape}: max|c| {np.abs(c).max():.4g}, nodes {err:.3g}, bound {bound:.3g}')
    assert back.dtype == np.float32 and err <= bound


def test_identity_transformation_is_the_node_grid():
    """linspace(-1, 1, n) through ((g + 1) * 0.5) * (n - 1) in float32 lands within 1 ulp of the nodes"""
    shape = (5, 6, 7)
    lin = [np.linspace(-1, 1, n, dtype=np.float32) for n in shape]
    z, y, x = np.meshgrid(*lin, indexing='ij')
    q = B.index_coordinates(np.stack((x, y, z)))
    for a, n in enumerate(shape):
        node = np.arange(n, dtype=np.float32).reshape([-1 if b == a else 1 for b in range(3)])
        assert np.abs(q[a] - node).max() <= n * 2.0 ** -23


def test_mirror_and_store_switch():
    assert B.mirror(np.array([-1, 0, 3, 4, 5]), 4).tolist() == [1, 0, 3, 2, 1]
    # 2 n - 2 <= 32 takes the exact start, 2 n - 2 = 34 the truncated series: both against the closed form of a constant line
    for n in (17, 18):
        c = B.prefilter_axis(np.ones((n, 1)), 0, np.float64)
        assert np.abs(c - 1.0).max() < 1e-14  # the spline of a constant has constant coefficients (6 / (4 + 1 + 1))
