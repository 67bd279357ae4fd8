"""The host side of the coarse-to-fine start, without a GPU: the properties of the numpy restatement of the three operators
(tests/_multires.py), every refusal and the defaults of `coarse_start_options`, and what the three operator wrappers hand to the
C ABI (through the recording stand-in of tests/test_residual_check_host.py)."""
import json
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import multires as M
from tests import _multires as S
from tests.test_residual_check_host import rec  # noqa: F401  (the fixture of the recording stand-in)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(9, 5), (44, 9), (13, 10), (12, 11), (70, 33), (3, 2), (5, 3), (4, 3), (128, 32), (7, 7), (2, 2)]  # (N, n)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize('N,n', PAIRS)
def test_rows_sum_to_one(N, n):
    R, P = S.restriction_matrix(N, n), S.prolongation_matrix(n, N)
    assert R.shape == (n, N) and P.shape == (N, n) and (R >= 0).all() and (P >= 0).all()
    assert np.abs(R.sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -53 * np.count_nonzero(R, axis=1).max()
    assert np.abs(P.sum(axis=1) - 1.0).max() <= 2.0 ** -52
    assert np.count_nonzero(P, axis=1).max() <= 2


@pytest.mark.parametrize('n', [2, 3, 7, 33])
def test_equal_extents_are_the_identity(n):
    assert (S.restriction_matrix(n, n) == np.eye(n)).all() and (S.prolongation_matrix(n, n) == np.eye(n)).all()
    assert (S.nearest_index(n, n) == np.arange(n)).all()
    x = np.random.default_rng(n).standard_normal((2, 1, n, n + 1, n + 2)).astype(np.float32)
    assert (S.restrict_image(x, x.shape[-3:]) == x).all() and (S.prolong_field(x, x.shape[-3:]) == x).all()


@pytest.mark.parametrize('n', [2, 3, 5, 17])
def test_full_weighting(n):
    R = S.restriction_matrix(2 * n - 1, n)
    want = np.zeros_like(R)
    for i in range(n):
        for k, w in ((2 * i - 1, 0.25), (2 * i, 0.5), (2 * i + 1, 0.25)):
            want[i, min(max(k, 0), 2 * n - 2)] += w
    assert (R == want).all()
    assert R[0, :2].tolist() == [0.75, 0.25] and R[-1, -2:].tolist() == [0.25, 0.75]
    if n > 2:
        assert R[1, 1:4].tolist() == [0.25, 0.5, 0.25]


@pytest.mark.parametrize('fine,coarse', [((9, 9, 9), (5, 5, 5)), ((44, 13, 12), (9, 10, 11)), ((3, 5, 70), (2, 3, 33))])
def test_a_constant_stays_constant(fine, coarse):
    down = S.restrict_image(np.full((1, 1, *fine), 0.7, np.float32), coarse)
    up = S.prolong_field(np.full((2, 3, *coarse), -1.3, np.float32), fine)
    assert down.shape == (1, 1, *coarse) and up.shape == (2, 3, *fine)
    assert np.abs(down - np.float64(np.float32(0.7))).max() <= 64 * 2.0 ** -53
    assert np.abs(up - np.float64(np.float32(-1.3))).max() <= 8 * 2.0 ** -53 * 1.3


def test_prolongation_reproduces_a_linear_ramp():
    # dyadic steps: exactly
    for coarse, fine in (((5, 5, 5), (9, 9, 9)), ((3, 5, 9), (9, 17, 33))):
        iz, iy, ix = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in coarse), indexing='ij')
        ramp = 0.5 + 2.0 * iz - 3.0 * iy + 0.25 * ix
        cz, cy, cx = np.meshgrid(*(np.arange(N) * (n - 1) / (N - 1) for n, N in zip(coarse, fine)), indexing='ij')
        assert (S.prolong_field(ramp, fine) == 0.5 + 2.0 * cz - 3.0 * cy + 0.25 * cx).all()
    # any step: to the rounding of the weights
    coarse, fine = (9, 10, 11), (44, 13, 12)
    iz, iy, ix = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in coarse), indexing='ij')
    cz, cy, cx = np.meshgrid(*(np.arange(N) * (n - 1) / (N - 1) for n, N in zip(coarse, fine)), indexing='ij')
    got, want = S.prolong_field(1.0 + iz - 2.0 * iy + 0.5 * ix, fine), 1.0 + cz - 2.0 * cy + 0.5 * cx
    assert np.abs(got - want).max() <= 32 * 2.0 ** -53 * np.abs(want).max()


def test_the_mask_rule_at_a_half_integer():
    assert S.fine_coordinate(1, 4, 3) == 1.5
    assert S.nearest_index(4, 3).tolist() == [0, 2, 3]  # floor(1.5 + 0.5) = 2: a half rounds up
    assert S.nearest_index(9, 5).tolist() == [0, 2, 4, 6, 8]
    m = np.arange(64, dtype=np.uint8).reshape(1, 1, 4, 4, 4)
    got = S.restrict_mask(m, (3, 3, 3))
    assert got.dtype == np.uint8 and got.shape == (1, 1, 3, 3, 3)
    assert got[0, 0, 1, 1, 1] == m[0, 0, 2, 2, 2] and got[0, 0, 2, 0, 1] == m[0, 0, 3, 0, 2]


# ---------------------------------------------------------------- the option
FINE = (32, 32, 32)
LEVELS = [{'dims': [9, 10, 11], 'no_iters': 4}, {'dims': [16, 16, 16], 'no_iters': 5, 'lr': 0.2}]


def cfg(coarse_start=None, **over):
    out = {'VI': False, 'MCMC_init': 'coarse', **over}
    if coarse_start is not None:
        out['coarse_start'] = coarse_start
    return out


def test_option_defaults():
    assert M.coarse_start_options({'VI': False, 'MCMC_init': 'identity'}, FINE, 'SVF_3D') is None
    assert M.coarse_start_options({'VI': True, 'MCMC_init': 'VI', 'coarse_start': None}, FINE, 'SVFFD_3D') is None
    assert M.coarse_start_options(cfg({'levels': LEVELS}), FINE, 'SVF_3D') == {'levels': [
        {'dims': (9, 10, 11), 'no_iters': 4, 'lr': None}, {'dims': (16, 16, 16), 'no_iters': 5, 'lr': 0.2}]}
    # a level may equal the next one, and the full grid on some axes but not on all
    ok = M.coarse_start_options(cfg({'levels': [{'dims': [16, 16, 16], 'no_iters': 1}, {'dims': [16, 16, 16], 'no_iters': 1},
                                                {'dims': [32, 32, 16], 'no_iters': 1}]}), FINE, 'SVF_3D')
    assert [lv['dims'] for lv in ok['levels']] == [(16, 16, 16), (16, 16, 16), (32, 32, 16)]
    shipped = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128_coarse.json')))
    base = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_ssd_l2_128.json')))
    got = M.coarse_start_options(shipped['trainer'], shipped['data_loader']['args']['dims'], shipped['transformation_module']['type'])
    assert [lv['dims'] for lv in got['levels']] == [(32, 32, 32), (64, 64, 64)] and all(lv['lr'] is None for lv in got['levels'])
    shipped['trainer'].pop('coarse_start')
    assert {**shipped, 'name': base['name'], 'trainer': {**shipped['trainer'], 'MCMC_init': 'identity'}} == base


one = lambda **kw: {'levels': [{'dims': [16, 16, 16], 'no_iters': 5, **kw}]}


@pytest.mark.parametrize('trainer,kind,message', [
    (cfg(), 'SVF_3D', r'trainer.MCMC_init = "coarse" needs trainer.coarse_start = \{"levels": \[...\]\}'),
    (cfg(one(), MCMC_init='identity'), 'SVF_3D',
     r"trainer.coarse_start is set but trainer.MCMC_init = 'identity'; it takes effect with MCMC_init = \"coarse\" only"),
    (cfg(True), 'SVF_3D', r'trainer.coarse_start must be \{"levels": \[\{"dims": \[d, h, w\], "no_iters": n, "lr": optional\}, ...\]\}, got True'),
    (cfg({**one(), 'colour': 1}), 'SVF_3D', r"trainer.coarse_start: unknown keys \['colour'\]; known: \['levels'\]"),
    (cfg(one(colour=1)), 'SVF_3D', r"trainer.coarse_start.levels\[0\]: unknown keys \['colour'\]; known: \['dims', 'no_iters', 'lr'\]"),
    (cfg({'levels': []}), 'SVF_3D', r'trainer.coarse_start.levels must be a list of 1 .. 4 levels, got \[\]'),
    (cfg({}), 'SVF_3D', r'trainer.coarse_start.levels must be a list of 1 .. 4 levels, got None'),
    (cfg({'levels': one()['levels'] * 5}), 'SVF_3D', r'trainer.coarse_start.levels must be a list of 1 .. 4 levels, got'),
    (cfg({'levels': [[16, 16, 16]]}), 'SVF_3D', r'trainer.coarse_start.levels\[0\] must be \{"dims": \[d, h, w\], "no_iters": n, "lr": optional\}'),
    (cfg({'levels': [{'dims': [16, 16, 16]}]}), 'SVF_3D', r'trainer.coarse_start.levels\[0\]: "no_iters" is missing'),
    (cfg({'levels': [{'no_iters': 3}]}), 'SVF_3D', r'trainer.coarse_start.levels\[0\]: "dims" is missing'),
    (cfg({'levels': [{'dims': [16, 16], 'no_iters': 3}]}), 'SVF_3D', r'trainer.coarse_start.levels\[0\].dims must be three integers \[d, h, w\], got \[16, 16\]'),
    (cfg({'levels': [{'dims': [16, 16, 16.0], 'no_iters': 3}]}), 'SVF_3D', r'levels\[0\].dims must be three integers'),
    (cfg({'levels': [{'dims': [16, 8, 16], 'no_iters': 3}]}), 'SVF_3D', r'trainer.coarse_start.levels\[0\]: dims \[16, 8, 16\] have an extent below 9'),
    (cfg({'levels': [{'dims': [16, 17, 16], 'no_iters': 3}, {'dims': [16, 16, 16], 'no_iters': 3}]}), 'SVF_3D',
     r'trainer.coarse_start.levels\[0\]: dims \[16, 17, 16\] exceed \[16, 16, 16\] of levels\[1\]'),
    (cfg({'levels': [{'dims': [16, 16, 33], 'no_iters': 3}]}), 'SVF_3D',
     r'trainer.coarse_start.levels\[0\]: dims \[16, 16, 33\] exceed \[32, 32, 32\] of the full grid'),
    (cfg({'levels': [{'dims': [16, 16, 16], 'no_iters': 3}, {'dims': [32, 32, 32], 'no_iters': 3}]}), 'SVF_3D',
     r'trainer.coarse_start.levels\[1\]: dims \[32, 32, 32\] are the full grid; the last level must be coarser'),
    (cfg(one(no_iters=0)), 'SVF_3D', r'trainer.coarse_start.levels\[0\]: no_iters must be >= 1, got 0'),
    (cfg(one(no_iters=2.0)), 'SVF_3D', r'trainer.coarse_start.levels\[0\].no_iters must be an integer, got 2.0'),
    (cfg(one(no_iters=True)), 'SVF_3D', r'trainer.coarse_start.levels\[0\].no_iters must be an integer, got True'),
    (cfg(one(lr=0)), 'SVF_3D', r'trainer.coarse_start.levels\[0\].lr must be a finite number > 0, got 0'),
    (cfg(one(lr=-0.1)), 'SVF_3D', r'trainer.coarse_start.levels\[0\].lr must be a finite number > 0, got -0.1'),
    (cfg(one(lr=float('nan'))), 'SVF_3D', r'trainer.coarse_start.levels\[0\].lr must be a finite number > 0, got nan'),
    (cfg(one(lr=float('inf'))), 'SVF_3D', r'trainer.coarse_start.levels\[0\].lr must be a finite number > 0, got inf'),
    (cfg(one(lr='0.1')), 'SVF_3D', r"trainer.coarse_start.levels\[0\].lr must be a finite number > 0, got '0.1'"),
    (cfg(one()), 'SVFFD_3D', r'trainer.coarse_start: SVFFD_3D is not supported \(B-spline coefficients are not samples'),
    (cfg(one(), VI=True), 'SVF_3D', r'trainer.coarse_start: trainer.VI must be false')])
def test_option_refusals(trainer, kind, message):
    with pytest.raises(ValueError, match=message):
        M.coarse_start_options(trainer, FINE, kind)


# ---------------------------------------------------------------- the wrappers, through the recording stand-in of the library
f32 = torch.float32
FINE5, COARSE5 = (6, 7, 8), (3, 4, 5)


def test_restrict_image_wrapper(rec):  # noqa: F811
    im = torch.zeros(2, 1, *FINE5)
    out = M.restrict_image(im, COARSE5)
    assert tuple(out.shape) == (2, 1, *COARSE5) and out.dtype == f32
    (name, a), = rec.calls
    assert name == 'irs_restrict_image' and a[0] == ((2, 1, *FINE5), f32, im.data_ptr()) and a[1:5] == [2, *FINE5]
    assert a[5] == ((2, 1, *COARSE5), f32, out.data_ptr()) and a[6:9] == list(COARSE5) and a[9] == 'stream'
    assert tuple(M.restrict_image(im, torch.tensor(COARSE5)).shape) == (2, 1, *COARSE5)  # dims may be a tensor or an array
    for call, message in ((lambda: M.restrict_image(im[:, 0], COARSE5), r'im must have shape \(C,1,D,H,W\), got \(2, 6, 7, 8\)'),
                          (lambda: M.restrict_image(im.expand(2, 3, *FINE5), COARSE5), r'im must have shape \(C,1,D,H,W\)'),
                          (lambda: M.restrict_image(im, (3, 4)), r'dims must be three integers \(d, h, w\), got \(3, 4\)'),
                          (lambda: M.restrict_image(im, (3, 4, 5.0)), r'dims must be three integers'),
                          (lambda: M.restrict_image(im.double(), COARSE5), 'expected torch.float32, got torch.float64')):
        with pytest.raises(L.IrsError, match=message):
            call()
    assert len(rec.calls) == 2  # the extents themselves are the library's to refuse


def test_restrict_mask_wrapper(rec):  # noqa: F811
    for dtype in (torch.bool, torch.uint8):
        mask = torch.ones(1, 1, *FINE5, dtype=dtype)
        out = M.restrict_mask(mask, COARSE5)
        assert tuple(out.shape) == (1, 1, *COARSE5) and out.dtype == dtype
        name, a = rec.calls[-1]
        assert name == 'irs_restrict_mask' and a[0] == ((1, 1, *FINE5), torch.uint8, mask.data_ptr()) and a[1:5] == [1, *FINE5]
        assert a[5] == ((1, 1, *COARSE5), torch.uint8, out.data_ptr()) and a[6:9] == list(COARSE5) and a[9] == 'stream'
    with pytest.raises(L.IrsError, match='mask must be bool or uint8, got torch.float32'):
        M.restrict_mask(torch.ones(1, 1, *FINE5), COARSE5)
    with pytest.raises(L.IrsError, match=r'mask must have shape \(C,1,D,H,W\)'):
        M.restrict_mask(torch.ones(*FINE5, dtype=torch.bool), COARSE5)
    assert len(rec.calls) == 2


def test_prolong_field_wrapper(rec):  # noqa: F811
    for ch in (1, 3):
        x = torch.zeros(2, ch, *COARSE5)
        out = M.prolong_field(x, FINE5)
        assert tuple(out.shape) == (2, ch, *FINE5) and out.dtype == f32
        name, a = rec.calls[-1]
        assert name == 'irs_prolong_field' and a[0] == ((2, ch, *COARSE5), f32, x.data_ptr()) and a[1:6] == [2, ch, *COARSE5]
        assert a[6] == ((2, ch, *FINE5), f32, out.data_ptr()) and a[7:10] == list(FINE5) and a[10] == 'stream'
    with pytest.raises(L.IrsError, match=r'x must have shape \(C,ch,D,H,W\), got \(3, 4, 5\)'):
        M.prolong_field(torch.zeros(*COARSE5), FINE5)
    with pytest.raises(L.IrsError, match='tensor must be contiguous'):
        M.prolong_field(torch.zeros(2, 3, 5, 4, 3).permute(0, 1, 4, 3, 2), FINE5)
    assert len(rec.calls) == 2


def test_restrict_pair(rec):  # noqa: F811
    fixed = {'im': torch.zeros(1, 1, *FINE5), 'mask': torch.ones(1, 1, *FINE5, dtype=torch.bool), 'seg': None}
    moving = {'im': torch.zeros(2, 1, *FINE5)}
    f, m = M.restrict_pair(fixed, moving, COARSE5)
    assert sorted(f) == ['im', 'mask'] and sorted(m) == ['im']
    assert tuple(f['im'].shape) == tuple(f['mask'].shape) == (1, 1, *COARSE5) and tuple(m['im'].shape) == (2, 1, *COARSE5)
    assert f['mask'].dtype == torch.bool
    assert [name for name, _ in rec.calls] == ['irs_restrict_image', 'irs_restrict_mask', 'irs_restrict_image']
    assert [a[0][2] for _, a in rec.calls] == [fixed['im'].data_ptr(), fixed['mask'].data_ptr(), moving['im'].data_ptr()]
