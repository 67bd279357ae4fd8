"""The coarse-to-fine start on the GPU: the three operators of ir_sgmcmc_amd/multires.py against the numpy restatement of
tests/_multires.py (which shares no code with the HIP path), the refusals of their C ABI, and the trainer's MCMC_init "coarse"
against a rebuild by hand from TransitionEngine and the operators.

Operator tolerance: the device and the restatement both round ONE double sum to float32.  The two sums differ by at most
taps * 2^-53 * max|input| (other order of the same products), which moves the rounded value only where the sum sits within that
of a rounding tie -- by one unit in the last place of a value of magnitude <= max|input|, i.e. at most 2^-23 max|input|.  So
|device - restatement| <= 2^-23 max|input|.  On dyadic inputs and dyadic weights nothing rounds and the two are EQUAL."""
import copy
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from ir_sgmcmc_amd import _lib as L
from ir_sgmcmc_amd import multires as M
from ir_sgmcmc_amd import ops
from ir_sgmcmc_amd.engine import TransitionEngine
from tests import _multires as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DYADIC = ((9, 9, 9), (5, 5, 5))    # N = 2 n - 1: the weights are dyadic
RAGGED = ((44, 13, 12), (9, 10, 11))  # no extent a multiple of the 64 x 4 block, a ratio per axis, several blocks along y
EDGE = ((3, 5, 70), (2, 3, 33))    # the extent-2 edge; a last axis longer than one wavefront on the fine side
EQUAL = ((5, 6, 70), (5, 6, 70))
SHAPES = [DYADIC, RAGGED, EDGE, EQUAL]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def values(shape, seed, dyadic):
    rng = np.random.default_rng(seed)
    if dyadic:
        return (rng.integers(-64, 65, shape) / 16.0).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def compare(name, got, want64, x, exact):
    want = want64.astype(np.float32)
    assert got.shape == want.shape and got.dtype == np.float32
    deviation, bound = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()), 2.0 ** -23 * float(np.abs(x).max())
    print(f'{name}: deviation {deviation:.3e}, bound {bound:.3e}{" (bit for bit)" if exact else ""}')
    if exact:
        assert (got.view(np.int32) == want.view(np.int32)).all(), name
    assert deviation <= bound, name


@pytest.mark.parametrize('fine,coarse', SHAPES)
@pytest.mark.parametrize('Cim', [1, 2])
def test_restrict_image_against_the_restatement(fine, coarse, Cim):
    exact = (fine, coarse) in (DYADIC, EQUAL)
    x = values((Cim, 1, *fine), sum(fine) + Cim, dyadic=(fine, coarse) == DYADIC)
    got = M.restrict_image(dev(x), coarse).cpu().numpy()
    compare(f'restrict {fine} -> {coarse}, Cim = {Cim}', got, S.restrict_image(x, coarse), x, exact)
    if (fine, coarse) == EQUAL:
        assert (got.view(np.int32) == x.view(np.int32)).all()


@pytest.mark.parametrize('fine,coarse', SHAPES)
@pytest.mark.parametrize('Cn,ch', [(1, 3), (2, 1)])
def test_prolong_field_against_the_restatement(fine, coarse, Cn, ch):
    exact = (fine, coarse) in (DYADIC, EQUAL)
    x = values((Cn, ch, *coarse), sum(coarse) + Cn, dyadic=(fine, coarse) == DYADIC)
    got = M.prolong_field(dev(x), fine).cpu().numpy()
    compare(f'prolong {coarse} -> {fine}, C = {Cn}, ch = {ch}', got, S.prolong_field(x, fine), x, exact)
    if (fine, coarse) == EQUAL:
        assert (got.view(np.int32) == x.view(np.int32)).all()


@pytest.mark.parametrize('fine,coarse', SHAPES + [((4, 4, 4), (3, 3, 3))])
@pytest.mark.parametrize('Cm,dtype', [(1, np.bool_), (2, np.uint8)])
def test_restrict_mask_against_the_restatement(fine, coarse, Cm, dtype):
    rng = np.random.default_rng(sum(fine) + Cm)
    m = rng.integers(0, 2, (Cm, 1, *fine)).astype(dtype) if dtype == np.bool_ else rng.integers(0, 256, (Cm, 1, *fine)).astype(dtype)
    got = M.restrict_mask(dev(m), coarse).cpu().numpy()
    want = S.restrict_mask(m, coarse)
    assert got.dtype == want.dtype == dtype and got.shape == (Cm, 1, *coarse) and (got == want).all()
    assert len(np.unique(want)) > 1  # the case tells one voxel from another


def test_determinism_and_chain_independence():
    fine, coarse = RAGGED
    x = dev(values((2, 1, *fine), 3, False))
    a, b = M.restrict_image(x, coarse), M.restrict_image(x, coarse)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a[1:].view(torch.int32), M.restrict_image(x[1:].contiguous(), coarse).view(torch.int32))
    v = dev(values((2, 3, *coarse), 4, False))
    a, b = M.prolong_field(v, fine), M.prolong_field(v, fine)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a[1:].view(torch.int32), M.prolong_field(v[1:].contiguous(), fine).view(torch.int32))


# ---------------------------------------------------------------- the C ABI refuses what it cannot do
def test_abi_refusals():
    lib = L.load()
    fine, coarse = (6, 6, 6), (4, 4, 4)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    im = torch.zeros(2, 1, *fine, device=DEV)
    mask = torch.ones(2, 1, *fine, device=DEV, dtype=torch.uint8)
    down = torch.full((2, 1, *coarse), 7.0, device=DEV)
    mdown = torch.full((2, 1, *coarse), 7, device=DEV, dtype=torch.uint8)
    field = torch.zeros(2, 3, *coarse, device=DEV)
    up = torch.full((2, 3, *fine), 7.0, device=DEV)

    def image(src=im, Cim=2, f=fine, out=down, c=coarse):
        return lib.irs_restrict_image(p(src), Cim, *f, p(out), *c, None)

    def msk(src=mask, Cm=2, f=fine, out=mdown, c=coarse):
        return lib.irs_restrict_mask(p(src), Cm, *f, p(out), *c, None)

    def prolong(src=field, Cn=2, ch=3, c=coarse, out=up, f=fine):
        return lib.irs_prolong_field(p(src), Cn, ch, *c, p(out), *f, None)

    cases = [(lambda: image(src=None), 'irs_restrict_image: null pointer'),
             (lambda: image(out=None), 'irs_restrict_image: null pointer'),
             (lambda: image(Cim=0), 'irs_restrict_image: Cim = 0 volumes, at least 1 needed'),
             (lambda: image(c=(1, 4, 4)), 'irs_restrict_image: coarse dims (1, 4, 4), every one >= 2 needed'),
             (lambda: image(f=(6, 1, 6), c=(4, 1, 4)), 'irs_restrict_image: fine dims (6, 1, 6), every one >= 2 needed'),
             (lambda: image(c=(4, 7, 4)), 'irs_restrict_image: coarse dims (4, 7, 4) exceed the fine dims (6, 6, 6) on axis 1'),
             (lambda: image(Cim=20000), 'irs_restrict_image: 20000 volumes of 4 planes are more than the 65535 rows of one launch'),
             (lambda: image(f=(1024, 1024, 1024)), 'irs_restrict_image: the fine volume must have fewer than 2^30 voxels'),
             (lambda: msk(src=None), 'irs_restrict_mask: null pointer'),
             (lambda: msk(out=None), 'irs_restrict_mask: null pointer'),
             (lambda: msk(Cm=-1), 'irs_restrict_mask: Cm = -1 volumes, at least 1 needed'),
             (lambda: msk(c=(4, 4, 0)), 'irs_restrict_mask: coarse dims (4, 4, 0), every one >= 2 needed'),
             (lambda: msk(c=(4, 4, 7)), 'irs_restrict_mask: coarse dims (4, 4, 7) exceed the fine dims (6, 6, 6) on axis 2'),
             (lambda: prolong(src=None), 'irs_prolong_field: null pointer'),
             (lambda: prolong(out=None), 'irs_prolong_field: null pointer'),
             (lambda: prolong(Cn=0), 'irs_prolong_field: C = 0 chains of ch = 3 channels, at least 1 each needed'),
             (lambda: prolong(ch=0), 'irs_prolong_field: C = 2 chains of ch = 0 channels, at least 1 each needed'),
             (lambda: prolong(c=(4, 1, 4)), 'irs_prolong_field: coarse dims (4, 1, 4), every one >= 2 needed'),
             (lambda: prolong(c=(7, 4, 4)), 'irs_prolong_field: coarse dims (7, 4, 4) exceed the fine dims (6, 6, 6) on axis 0'),
             (lambda: prolong(Cn=4000, ch=3), 'irs_prolong_field: 12000 volumes of 6 planes are more than the 65535 rows of one launch')]
    for call, message in cases:
        assert call() != 0 and lib.irs_last_error().decode() == message, (lib.irs_last_error().decode(), message)
    torch.cuda.synchronize()
    assert (down == 7.0).all() and (mdown == 7).all() and (up == 7.0).all()  # nothing was launched
    assert image() == 0 and msk() == 0 and prolong() == 0
    torch.cuda.synchronize()
    assert (down == 0.0).all() and (mdown == 1).all() and (up == 0.0).all()


# ---------------------------------------------------------------- the trainer
SSD, GMM = 'synthetic_ssd_l2_128.json', 'synthetic_gmm_lognormal.json'
N = 32
ONE = [{'dims': [16, 16, 16], 'no_iters': 5}]
TWO = [{'dims': [9, 10, 11], 'no_iters': 4, 'lr': 0.2}, {'dims': [16, 16, 16], 'no_iters': 4}]


def make_trainer(tmp_path, name, levels, **trainer_over):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    cfg = json.load(open(os.path.join(ROOT, 'configs', name)))
    cfg['trainer']['save_dir'] = str(tmp_path)
    cfg['data_loader']['args']['dims'] = [N, N, N]
    cfg['trainer'].update(VI=False, MCMC=True, no_iters_VI=0, no_samples_VI_test=0, **trainer_over)
    if levels is not None:
        cfg['trainer'].update(MCMC_init='coarse', coarse_start={'levels': levels})
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    dl = config.init_data_loader()
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, dl, config.init_losses(), tm, rm, config.init_metrics(), device=DEV), dl


def initialise(t, dl):
    """_run_model up to the point where _SGLD_init is due"""
    fixed, moving, vp = next(iter(dl))
    fixed = {k: v.to(DEV) for k, v in fixed.items()}
    moving = {k: v.to(DEV) for k, v in moving.items()}
    t._engine_init(fixed, moving)
    t._GMM_init(fixed, moving, vp)
    return vp


def rebuild(t, levels):
    """the flow of the coarse start, by hand from TransitionEngine and the operators; reads the trainer, changes nothing of it"""
    base = t._engine_config()
    data_loss, reg_loss = t.losses['data']['loss'], t.losses['reg']['loss']
    v = None
    for no, level in enumerate(levels):
        d = tuple(level['dims'])
        cfg = dataclasses.replace(base, dims=d, lr=level.get('lr', base.lr), seed=base.seed + 1 + no)
        engine = TransitionEngine(cfg, DEV)
        fixed, moving = engine.prepare(*M.restrict_pair(t._fixed, t._moving, d))
        st = engine.state()
        if type(data_loss).__name__ == 'GMM':
            for k in range(data_loss.no_components):
                st.gmm_log_std[k], st.gmm_logits[k] = float(data_loss.log_std[k].detach()), float(data_loss.logits[k].detach())
        if type(reg_loss).__name__ == 'RegLoss_L2':
            st.reg_param[0] = float(reg_loss.log_w_reg.detach())
        engine.set_state(st)  # a log-normal regulariser keeps the (loc, log_scale) of the level's own degrees of freedom
        v = torch.zeros(t.no_chains, 3, *d, device=DEV) if v is None else M.prolong_field(v, d)
        engine.gmm_init(fixed, moving, None if no == 0 else v[:1])
        for it in range(level['no_iters']):
            engine.transition(fixed, moving, v)
            if it == 0:
                engine.scalars()
        engine.flush()
        del engine
    return M.prolong_field(v, (N, N, N))


bits = lambda x: x.view(torch.int32)


@pytest.mark.parametrize('levels', [ONE, TWO])
def test_trainer_start_is_the_hand_rebuild(tmp_path, levels):
    t, dl = make_trainer(tmp_path / 'a', SSD, levels, no_chains=2)
    vp = initialise(t, dl)
    want = rebuild(t, levels)
    t._SGLD_init(vp)
    assert t.v_curr_state.shape == (2, 3, N, N, N) and t._sigma is None and torch.isfinite(t.v_curr_state).all()
    assert torch.equal(bits(t.v_curr_state), bits(want))
    assert not torch.equal(t.v_curr_state[0], t.v_curr_state[1])  # the chains drew their own noise
    assert float(t.v_curr_state.abs().max()) > 0
    s = t.coarse_summary
    assert [e['dims'] for e in s] == [tuple(lv['dims']) for lv in levels] and [e['no_iters'] for e in s] == [lv['no_iters'] for lv in levels]
    assert [e['lr'] for e in s] == [lv.get('lr', 0.4) for lv in levels]
    for e in s:
        assert set(e) == {'dims', 'no_iters', 'lr', 'data_term_first', 'data_term_last', 'seconds'} and e['seconds'] > 0
        assert len(e['data_term_first']) == len(e['data_term_last']) == 2
        assert all(np.isfinite(e['data_term_first'])) and all(np.isfinite(e['data_term_last']))
    # a second trainer of the same config starts at the same bits
    u, dl_u = make_trainer(tmp_path / 'b', SSD, levels, no_chains=2)
    u._SGLD_init(initialise(u, dl_u))
    assert torch.equal(bits(u.v_curr_state), bits(t.v_curr_state))
    assert [e['data_term_last'] for e in u.coarse_summary] == [e['data_term_last'] for e in s]


def test_trainer_start_of_a_mixture_with_a_lognormal_regulariser(tmp_path):
    t, dl = make_trainer(tmp_path, GMM, ONE, no_chains=2)
    assert type(t.losses['data']['loss']).__name__ == 'GMM' and type(t.losses['reg']['loss']).__name__ == 'RegLoss_LogNormal'
    vp = initialise(t, dl)
    want = rebuild(t, ONE)
    t._SGLD_init(vp)
    assert torch.equal(bits(t.v_curr_state), bits(want)) and float(t.v_curr_state.abs().max()) > 0
    assert torch.isfinite(t.losses['data']['loss'].log_std).all()  # re-seeded from the residuals of the prolonged field


def test_run_checkpoint_and_resume(tmp_path):
    kw = dict(no_chains=2, no_iters_burn_in=2, no_samples_MCMC=8, log_period_MCMC=4, checkpoint_period=6)
    a, _ = make_trainer(tmp_path / 'a', SSD, TWO, **kw)
    a.run()
    assert [e['dims'] for e in a.coarse_summary] == [(9, 10, 11), (16, 16, 16)]
    ck = a.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt'
    b, _ = make_trainer(tmp_path / 'b', SSD, TWO, resume=str(ck), **kw)
    b.run()
    assert b.coarse_summary == []  # the checkpoint supplied v: no level ran
    assert torch.equal(bits(a.v_curr_state), bits(b.v_curr_state))
    # another start: the same metric keys and checkpoint keys, and no summary
    off, _ = make_trainer(tmp_path / 'off', SSD, None, MCMC_init='identity', **kw)
    off.run()
    assert off.coarse_summary is None and off.coarse_options is None
    assert set(off.metrics.result()) == set(a.metrics.result())
    sd = lambda t: torch.load(t.config.save_dirs['checkpoints'] / 'checkpoint_0000006.pt', map_location='cpu', weights_only=True)
    assert set(sd(off)) == set(sd(a))
    assert not torch.equal(a.v_curr_state, off.v_curr_state)


def test_the_coarse_start_is_closer_than_the_identity(tmp_path):
    """SSD at 32^3, one level of 16^3 with 40 transitions: m(v) = the masked mean square of fixed - warp(moving, exp(S v)) at the
    start against m(0).  The CPU oracle gave ratios of 0.42 .. 0.50 over five noise seeds; the device draws other noise, so the
    bound sits halfway between the worst of them and no improvement at all."""
    t, dl = make_trainer(tmp_path, SSD, [{'dims': [16, 16, 16], 'no_iters': 40}])
    t._SGLD_init(initialise(t, dl))
    kernel = ops.sobolev_kernel_1d(t.Sobolev_s, t.Sobolev_lambda)
    fixed, moving, mask = t._fixed['im'], t._moving['im'], t._fixed['mask']

    def m(v):
        transformation = ops.svf_exp_fwd(ops.perturb_smooth(v, kernel, tau=None), t._engine_config().no_steps)[0]
        diff = (fixed - ops.warp(moving, transformation))[mask]
        return float((diff.double() ** 2).mean())

    start, identity = m(t.v_curr_state), m(torch.zeros_like(t.v_curr_state))
    print(f'm(coarse start) = {start:.6f}, m(0) = {identity:.6f}, ratio {start / identity:.4f} (bound 0.75)')
    assert start < 0.75 * identity
