"""The bending-energy prior without a GPU: the float64 closed form of tests/_bending.py against the fixture computed with the
reference's own GradientOperator applied twice (tests/golden/make_golden_bending.py), the interior stencil, and the host-side
plumbing -- the operator's name resolves, an engine configuration maps it, the C struct carries it where the padding was."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd.engine import EngineConfig, irs_config
from ir_sgmcmc_amd.model.loss import RegLoss_L2, RegLoss_LogNormal, RegLoss_Student
from ir_sgmcmc_amd.utils.diff_op import DifferentialOperator, GradientOperator, HessianOperator
from tests import _bending as B

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(2, 3, 3, 3, 3), (1, 3, 2, 5, 6), (2, 3, 7, 9, 11)]


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'bending_ops.npz'))


@pytest.mark.parametrize('i', range(len(SHAPES)))
def test_closed_form_is_the_gradient_operator_applied_twice(golden, i):
    v = torch.from_numpy(golden[f'v_{i}'])
    assert tuple(v.shape) == SHAPES[i] and v.dtype == torch.float64
    y, y_ref = B.energy(v), torch.from_numpy(golden[f'y_{i}'])
    assert float(((y - y_ref).abs() / y_ref).max()) <= 1e-12
    g, g_ref = B.grad(v), torch.from_numpy(golden[f'g_{i}'])
    assert float((g - g_ref).abs().max()) <= 1e-12 * float(g_ref.abs().max())
    assert bool((B.grad_abs(v) >= g.abs()).all())  # the magnitude bound dominates the value it bounds


def test_interior_stencil():
    """centre 84, six axis neighbours -24, six at distance two +2, twelve in-plane diagonals +4: 288 in absolute value"""
    v = torch.zeros(1, 3, 9, 9, 9, dtype=torch.float64)
    v[0, 1, 4, 4, 4] = 1.0
    g, ga = B.grad(v), B.grad_abs(v)
    assert float(g[0, 0].abs().max()) == 0.0 and float(g[0, 2].abs().max()) == 0.0  # components do not couple
    g = g[0, 1]
    assert g[4, 4, 4] == 84 and g[4, 4, 5] == g[4, 3, 4] == g[5, 4, 4] == -24 and g[4, 4, 6] == g[2, 4, 4] == 2
    assert g[4, 5, 5] == g[3, 4, 5] == g[5, 3, 4] == 4 and g[5, 5, 5] == 0 and g[4, 4, 7] == 0
    assert float(g.abs().sum()) == 288.0 and int((g != 0).sum()) == 25
    assert torch.equal(ga[0, 1], g.abs())
    # an affine field carries no bending energy, unlike the first-order energy
    zz, yy, xx = torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in (5, 6, 7)], indexing='ij')
    affine = torch.stack([1.0 + 2.0 * xx - yy, 0.5 * zz, xx + yy + zz]).unsqueeze(0)
    assert float(B.energy(affine)) == 0.0


def test_name_resolves():
    assert isinstance(DifferentialOperator.from_string('HessianOperator'), HessianOperator)
    assert isinstance(DifferentialOperator.from_string('GradientOperator'), GradientOperator)
    with pytest.raises(ValueError):
        DifferentialOperator.from_string('FourierOperator')
    for loss in (RegLoss_L2(1.4, diff_op='HessianOperator', dims=(8, 8, 8)), RegLoss_LogNormal(1.0, diff_op='HessianOperator', dims=(8, 8, 8)),
                 RegLoss_Student(diff_op='HessianOperator', dims=(8, 8, 8))):
        assert isinstance(loss.diff_op, HessianOperator)


def test_engine_config_maps_the_operator():
    assert EngineConfig(dims=(8, 8, 8)).diff_op == 'GradientOperator'
    assert irs_config(EngineConfig(dims=(8, 8, 8))).diff_op == 0 == L.IRS_DIFF_GRADIENT
    assert irs_config(EngineConfig(dims=(8, 8, 8), diff_op='HessianOperator')).diff_op == 1 == L.IRS_DIFF_HESSIAN
    with pytest.raises(ValueError, match='diff_op'):
        irs_config(EngineConfig(dims=(8, 8, 8), diff_op='FourierOperator'))


def test_field_sits_in_the_padding_hole():
    """offset 212, between reg_scale_prior_scale and the doubles: the size and every other offset are what they were"""
    assert L.IrsConfig.diff_op.offset == 212 and L.IrsConfig.diff_op.size == 4
    assert L.IrsConfig.reg_scale_prior_scale.offset == 208 and L.IrsConfig.w_reg_prior_shape.offset == 216
    assert L.IrsConfig.seed.offset == 232 and C.sizeof(L.IrsConfig) == 240


def test_slab_engine_refuses_the_operator_before_it_creates_anything():
    from ir_sgmcmc_amd.slab import SlabEngine
    with pytest.raises(L.IrsError, match='diff_op'):
        SlabEngine(EngineConfig(dims=(16, 16, 16), diff_op='HessianOperator'), 'cuda:0')


def test_config_is_the_l2_config_with_the_operator_swapped():
    import json
    root = os.path.dirname(HERE)
    a = json.load(open(os.path.join(root, 'configs', 'synthetic_ssd_l2_128.json')))
    b = json.load(open(os.path.join(root, 'configs', 'synthetic_ssd_bending_128.json')))
    assert b['reg_loss']['args']['diff_op'] == 'HessianOperator' and b['name'] == 'synthetic_ssd_bending_128'
    for cfg in (a, b):
        cfg.pop('name')
        cfg['reg_loss']['args'].pop('diff_op')
        cfg['reg_loss']['args'].pop('w_reg')
    assert a == b
