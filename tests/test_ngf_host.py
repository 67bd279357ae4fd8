"""The two restatements of the NGF data term (tests/_ngf.py) and everything about the feature that needs no device: the float64
gradient against autograd of the definition and against central differences, the float32 restatement inside the derived bound, the
mistakes that bound is there to catch, the edge parameters, config parsing, the refusals of the engine, the trainer and the slab
engine, the ABI symbols and the synthetic loader's moving_bias."""
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from tests import _ngf as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SHAPES = [(2, 2, 2), (3, 3, 3), (2, 5, 6), (1, 4, 4), (5, 6, 70)]
EPS = (0.3, 0.41)


def case(dims, C=2):
    fixed, moving = N.images(dims, C)
    return fixed, moving, N.upstream(dims, C)


@pytest.mark.parametrize('dims', SHAPES)
def test_gradient_equals_autograd(dims):
    """grad^T through the dense matrices against float64 autograd of the definition: 1e-12 of the largest element"""
    fixed, moving, u = case(dims)
    ref = N.reference(fixed, moving, u, *EPS)
    ga = N.autograd_gradient(fixed, moving, u, *EPS)
    top = float(ref['g'].abs().max())
    dev = float((ga - ref['g']).abs().max())
    print(f'{dims}: max|g| {top:.4g}, deviation {dev:.3g}')
    assert top > 0.1 and dev <= 1e-12 * top
    assert float(ref['d'].min()) >= 0.0 and float(ref['d'].max()) <= 1.0


def test_gradient_equals_central_differences():
    """deviation <= 1e-6 max|g| at step 1e-5 in float64: the truncation of the differences is O(h^2 d'''), the rounding
    O(1e-16 loss / h)"""
    dims = (3, 4, 5)
    fixed, moving, u = case(dims, 1)
    ref = N.reference(fixed, moving, u, *EPS)
    loss = lambda m: float(N.loss_sums(u, N.terms(fixed, m, u, *EPS)['d'])[0])
    h, m64 = 1e-5, moving.to(F64)
    fd = torch.zeros(m64.numel(), dtype=F64)
    for i in range(m64.numel()):
        mp, mn = m64.clone().reshape(-1), m64.clone().reshape(-1)
        mp[i] += h
        mn[i] -= h
        fd[i] = (loss(mp.reshape(m64.shape)) - loss(mn.reshape(m64.shape))) / (2 * h)
    top = float(ref['g'].abs().max())
    dev = float((fd - ref['g'].reshape(-1)).abs().max())
    print(f'max|g| {top:.4g}, deviation {dev:.3g}')
    assert top > 0.1 and dev <= 1e-6 * top


def shares(got, ref):
    """the largest share of the bound that `got` (dict d, coef, g of float32) uses, per output; an element with a zero bound (a
    coefficient on an axis of length 1) must be exact"""
    out = {}
    rows = [('d', got['d'], ref['d'], ref['tol']['d']), ('g', got['g'], ref['g'], ref['tol']['g'])]
    rows += [(f'c{i}', got['coef'][:, i:i + 1], ref['c'][i], ref['tol']['c'][i]) for i in range(3)]
    for name, x, y, tol in rows:
        y, tol = torch.broadcast_tensors(y, x)[0], torch.broadcast_tensors(tol, x)[0]
        dev = (x.to(F64) - y).abs()
        assert bool((dev[tol == 0] == 0).all()), name
        out[name] = float((dev[tol > 0] / tol[tol > 0]).max()) if bool((tol > 0).any()) else 0.0
    return out


@pytest.mark.parametrize('dims', SHAPES)
def test_float32_restatement_is_inside_the_bound(dims):
    """the float32 restatement uses at most 0.25 of the first-order bound on these images (d 0.25, c 0.24, g 0.12 at (5, 6, 70))"""
    fixed, moving, u = case(dims)
    ref = N.reference(fixed, moving, u, *EPS)
    used = shares(N.restate32(fixed, moving, u, *EPS), ref)
    print(dims, {k: round(v, 3) for k, v in used.items()})
    assert max(used.values()) <= 1.0


@pytest.mark.parametrize('dims', [(3, 3, 3), (5, 6, 70)])
@pytest.mark.parametrize('mistake', N.MISTAKES)
def test_each_mistake_exceeds_the_bound(mistake, dims):
    fixed, moving, u = case(dims)
    ref = N.reference(fixed, moving, u, *EPS)
    wrong = N.gradient(N.terms(fixed, moving, u, *EPS, mistake=mistake)['c'], mistake)
    factor = float(((wrong - ref['g']).abs() / ref['tol']['g']).max())
    print(f'{mistake} at {dims}: {factor:.3g} x the bound')
    assert factor > 1000.0


def test_dropped_fold_moves_the_face_rows():
    """leaving the fold out of the face rows moves g there by O(1) of max|g|: a missing fold cannot hide"""
    fixed, moving, u = case((5, 6, 70))
    ref = N.reference(fixed, moving, u, *EPS)
    wrong = N.gradient(ref['c'], 'drop_fold_low')
    moved = (wrong - ref['g']).abs()
    assert float(moved[..., 0, :].max()) > 0.1 * float(ref['g'].abs().max()) and float(moved[..., 1:, :].max()) == 0.0


def test_flat_and_identical_images():
    flat = torch.full((1, 1, 3, 4, 5), 0.75)
    _, moving, _ = case((3, 4, 5), 1)
    for f, m in ((flat, moving), (moving, flat), (flat, flat)):
        out = N.restate32(f, m, None, *EPS)
        assert bool((out['d'] == 1.0).all()) and not bool(out['g'].any()) and not bool(out['coef'].any())
    same = N.restate32(moving, moving, None, *EPS)
    assert bool(torch.isfinite(same['g']).all()) and float(same['d'].min()) >= 0.0 and float(same['d'].max()) < 1.0


def test_edge_parameters():
    from ir_sgmcmc_amd.ngf import ngf_edge_parameters
    fixed, moving = N.images((5, 6, 7), 1)
    mask = torch.rand(1, 1, 5, 6, 7, generator=torch.Generator().manual_seed(2)) < 0.6

    def mean_norm(im, mk=None):
        x = im[0, 0].numpy().astype(np.float64)
        g = []
        for ax in range(3):
            i = np.arange(x.shape[ax])
            g.append(0.5 * (np.take(x, np.minimum(i + 1, x.shape[ax] - 1), ax) - np.take(x, np.maximum(i - 1, 0), ax)))
        nrm = np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)
        return float(nrm.mean() if mk is None else nrm[mk[0, 0].numpy()].mean())

    ef, em = ngf_edge_parameters(fixed, moving)
    assert abs(ef - mean_norm(fixed)) <= 1e-12 * ef and abs(em - mean_norm(moving)) <= 1e-12 * em
    ef, em = ngf_edge_parameters(fixed, moving, mask, None)
    assert abs(ef - mean_norm(fixed, mask)) <= 1e-12 * ef and abs(em - mean_norm(moving)) <= 1e-12 * em
    ef, em = ngf_edge_parameters(fixed, moving, mask, mask)
    assert abs(em - mean_norm(moving, mask)) <= 1e-12 * em and isinstance(ef, float)


def test_switch_value_and_abi_symbols():
    assert (L.IRS_DATA_GMM_LCC, L.IRS_DATA_SSD, L.IRS_DATA_LNCC, L.IRS_DATA_MI, L.IRS_DATA_NGF) == (0, 1, 3, 4, 5)
    header = open(os.path.join(ROOT, 'include', 'irsgmcmc.h')).read()
    exports = open(os.path.join(ROOT, 'ir_sgmcmc_amd', 'csrc', 'exports.map')).read()
    assert re.search(r'IRS_DATA_NGF = 5\b', header) and 'global: irs_*;' in exports
    for name, nargs in (('irs_ngf_fwd', 16), ('irs_ngf_bwd', 7), ('irs_ngf_set', 4)):
        assert re.search(r'\bint %s\(' % name, header), name
        assert len(L.SIGNATURES[name]) == nargs
    device = open(os.path.join(ROOT, 'ir_sgmcmc_amd', 'csrc', 'ngf_device.h')).read()
    assert '__fdiv_rn' in device and 'fmaf' not in device


def test_config_resolves_the_class():
    from ir_sgmcmc_amd.model import loss as model_loss
    from ir_sgmcmc_amd.parse_config import ConfigParser
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ngf_l2_128.json')))
    args = cfg['data_loader']['args']
    assert args['moving_contrast'] == 'invert' and args['moving_bias'] == 0.5 and cfg['virtual_decimation'] is False
    mi = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_mi_l2_128.json')))
    for key in ('reg_loss', 'transformation_module', 'optimizer_SG_MCMC', 'Sobolev_grad', 'trainer'):
        assert cfg[key] == mi[key], key
    cfg['trainer']['save_dir'] = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'ngf_host_config')
    config = ConfigParser.from_dict(cfg, timestamp='t')
    loss = config.init_losses()['data']['loss']
    assert isinstance(loss, model_loss.NGF) and loss.weight == cfg['data_loss']['args']['weight']
    assert loss.fixed_eps is None and loss.moving_eps is None
    assert float(loss(torch.full((2, 3), 0.5, dtype=torch.float64))) == pytest.approx(loss.weight * 3.0, rel=1e-12)
    dl = config.init_data_loader()
    assert dl.moving_contrast == 'invert' and dl.moving_bias == 0.5


def test_engine_config_and_refusals():
    from ir_sgmcmc_amd.engine import DATA_LOSSES, EngineConfig, irs_config
    from ir_sgmcmc_amd.slab import SlabEngine
    from ir_sgmcmc_amd.trainer.trainer import ENGINE_DATA_LOSSES, engine_data_loss, ngf_refusals
    from ir_sgmcmc_amd.model import loss as model_loss
    # every data-loss class of the package is known to the engine, and an unknown one is refused, not run as SSD
    classes = [n for n, c in vars(model_loss).items() if isinstance(c, type) and issubclass(c, model_loss.DataLoss) and c is not model_loss.DataLoss]
    assert sorted(classes) == sorted(ENGINE_DATA_LOSSES) == sorted(DATA_LOSSES) and [engine_data_loss(k) for k in classes] == classes
    with pytest.raises(ValueError, match="data_loss.type 'NCC' is not wired"):
        engine_data_loss('NCC')
    assert DATA_LOSSES['NGF'] == L.IRS_DATA_NGF
    ec = EngineConfig(dims=(16, 16, 16), data_loss='NGF', virtual_decimation=False)
    assert (ec.ngf_weight, ec.ngf_fixed_eps, ec.ngf_moving_eps) == (1.0, None, None)
    assert irs_config(ec).data_loss == 5
    with pytest.raises(ValueError, match='not wired'):
        irs_config(EngineConfig(dims=(16, 16, 16), data_loss='NGFx'))
    with pytest.raises(L.IrsError, match='NGF data term is not supported on z-slabs'):
        SlabEngine(EngineConfig(dims=(16, 16, 16), data_loss='NGF', virtual_decimation=False), 'cpu', None)
    ngf_refusals(False, None)
    with pytest.raises(ValueError, match='virtual decimation'):
        ngf_refusals(True, None)
    with pytest.raises(ValueError, match='residual_check'):
        ngf_refusals(False, {'bins': 32})
    src = open(os.path.join(ROOT, 'ir_sgmcmc_amd', 'csrc', 'slab.hip')).read()
    assert 'cfg->data_loss == IRS_DATA_NGF' in src and 'the NGF data term is not supported on z-slabs' in src


# sha256 over the bytes of fixed im, mask, seg, moving im, mask, seg of synthetic_pair((12, 10, 14), seed=3, moving_contrast=X) as the
# function returned them before it had a `moving_bias` argument
PAIR_DIGESTS = {None: 'c0fb0144285c61424dbfe33d139f7e516afba1c727374cb8817cf66925301f21', 'invert': 'e219113d0d8973b5142a1bb42375159a33665a36738a3a9ad2cb24c0f9ee1a1b'}


def pair_digest(fixed, moving):
    h = hashlib.sha256()
    for t in (fixed, moving):
        for k in ('im', 'mask', 'seg'):
            h.update(t[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def test_moving_bias():
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    from ir_sgmcmc_amd.data_loader.data_loaders import SyntheticDataLoader
    dims = (12, 10, 14)
    for contrast, digest in PAIR_DIGESTS.items():
        f0, m0 = synthetic_pair(dims, seed=3, moving_contrast=contrast)
        f1, m1 = synthetic_pair(dims, seed=3, moving_contrast=contrast, moving_bias=None)
        assert pair_digest(f0, m0) == digest == pair_digest(f1, m1)            # absent: bit for bit as it always was
    f0, m0 = synthetic_pair(dims, seed=3, moving_contrast='invert')
    fb, mb = synthetic_pair(dims, seed=3, moving_contrast='invert', moving_bias=0.5)
    assert torch.equal(fb['im'], f0['im']) and torch.equal(mb['mask'], m0['mask']) and torch.equal(mb['seg'], m0['seg'])
    zn = torch.linspace(-1, 1, dims[0]).view(dims[0], 1, 1)
    assert torch.allclose(mb['im'] / m0['im'], torch.exp(0.5 * zn).expand(dims).unsqueeze(0), rtol=1e-6)   # exp(a z_n), after the contrast map
    for bad in ('0.5', True, float('nan')):
        with pytest.raises(ValueError, match='moving_bias'):
            synthetic_pair(dims, moving_bias=bad)
    _, moving, _ = next(iter(SyntheticDataLoader(dims, seed=3, moving_contrast='invert', moving_bias=0.5)))
    assert torch.equal(moving['im'][0], mb['im'])
    _, moving, _ = next(iter(SyntheticDataLoader(dims, seed=3)))
    assert torch.equal(moving['im'][0], synthetic_pair(dims, seed=3)[1]['im'])
