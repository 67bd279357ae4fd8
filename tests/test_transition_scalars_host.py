"""Host side of tests/test_gpu_transition_scalars.py: the fp64 restatement of the three closing stages of a transition
(tests/_transition_scalars.py) against the CPU oracle run in float64, the proof that the tolerances of the GPU test see the
mistakes they are for (each beaten 100x by a deliberate mistake in the restatement), and the conditioning of the hand-set mixture
the GPU test starts from."""
import math

import pytest
import torch

from oracle import OracleChain, OracleConfig
from oracle import ops as O
from tests import _transition_scalars as R

F64 = torch.float64
DIMS = (7, 13, 70)


def hyper_from_oracle(oc):
    """exact doubles, except where oracle/ops.py itself pins float32 (shape and rate of the Gamma log-densities)"""
    shape = 0.5 * oc.dof
    wprior = O.student_params(*oc.student) if oc.reg_loss == 'RegLoss_Student' else (R.f32(shape), R.f32(1.0 / shape))
    return R.Hyper(K=oc.gmm_components, data_loss=oc.data_loss, virtual_decimation=oc.virtual_decimation, ssd_inv_sigma=1.0 / oc.ssd_sigma,
                   gmm_lr=(oc.gmm_lr_log_std, oc.gmm_lr_logits), gmm_lr_decay=oc.gmm_lr_decay, scale_prior=oc.scale_prior,
                   conc=[oc.dirichlet_alpha] * oc.gmm_components, reg_loss=oc.reg_loss, reg_learnable=oc.reg_learnable, dof=oc.dof,
                   reg_lr=oc.reg_lr, reg_lr_decay=oc.reg_lr_decay, loc_prior_shape=R.f32(0.5 * oc.reg_loc_prior_nu * oc.dof),
                   loc_prior_rate=R.f32(0.5 * oc.reg_loc_prior_nu * oc.w_reg), reg_scale_prior=oc.reg_scale_prior, w_reg_prior=wprior, lr=oc.lr)


def adam_state(adam, n):
    st = [adam.state[i] for i in range(n)]
    return torch.stack([s['m'].detach().clone().reshape(-1) for s in st]), torch.stack([s['v'].detach().clone().reshape(-1) for s in st]), [s['step'] for s in st]


def reg_params(orc):
    if orc.cfg.reg_loss == 'RegLoss_LogNormal':
        return [float(orc.loc), float(orc.log_scale)]
    return [float(orc.log_w_reg)] if orc.cfg.reg_loss == 'RegLoss_L2' else [math.log(orc.cfg.w_reg)]


def oracle64(oc, zero_moving=False, sigma=None):
    """one float64 transition of the oracle -> (outputs, mixture / regulariser state before, after, inputs)"""
    fixed, moving, v0, eps, unif = R.make_inputs(oc.dims, oc.no_chains)
    torch.set_default_dtype(F64)
    try:
        C = oc.no_chains
        cast = lambda d: {k: (v.to(F64) if v.is_floating_point() else v).expand(C, *v.shape[1:]).contiguous() for k, v in d.items()}
        fixed, moving = cast(fixed), cast(moving)
        if zero_moving:
            moving['im'] = torch.zeros_like(moving['im'])
        orc = OracleChain(oc, v0=v0.to(F64), sigma=sigma)
        orc.init_gmm(fixed, moving)
        before = {'log_std': orc.log_std.detach().clone(), 'logits': orc.logits.detach().clone(), 'reg_param': reg_params(orc)}
        if oc.data_loss == 'GMM':
            before['m'], before['v'], before['step'] = adam_state(orc.adam_gmm, 2)
        o = orc.transition(fixed, moving, eps.to(F64), unif.to(F64))
        after = {'reg_param': reg_params(orc)}
        if oc.data_loss == 'GMM':
            after['m'], after['v'], after['step'] = adam_state(orc.adam_gmm, 2)
        if orc.adam_reg is not None:
            n = len(orc.adam_reg.state)
            after['reg_m'], after['reg_v'], _ = adam_state(orc.adam_reg, n)
        return o, before, after, fixed, v0.to(F64)
    finally:
        torch.set_default_dtype(torch.float32)


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize('K', [4, 6])
def test_mixture_stage_is_the_oracle_in_float64(K):
    oc = OracleConfig(dims=DIMS, no_chains=2, gmm_components=K, lr=0.05)
    o, before, after, fixed, _ = oracle64(oc)
    h = hyper_from_oracle(oc)
    recs, final = R.mixture_stage(o['residuals'], fixed['mask'], before, h, round_params=False)
    for c, r in enumerate(recs):
        assert r['n'] == float(fixed['mask'][c].sum())
        assert rel(r['alpha'], o['alpha'][c]) < 1e-10
        assert rel(r['data_term'], o['data'][c]) < 1e-10
        assert rel(r['log_std'], o['gmm_log_std'][c]) < 1e-10 and rel(r['logits'], o['gmm_logits'][c]) < 1e-10
    assert rel(final['m'], after['m']) < 1e-10 and rel(final['v'], after['v']) < 1e-10
    assert final['step'] == after['step'] == [27, 27]


@pytest.mark.parametrize('reg_loss,learnable', [('RegLoss_L2', False), ('RegLoss_L2', True), ('RegLoss_LogNormal', True), ('RegLoss_LogNormal', False),
                                                ('RegLoss_Student', False), ('RegLoss_LogNormal_L2', False)])
def test_regulariser_stage_and_update_are_the_oracle_in_float64(reg_loss, learnable):
    """moving image identically zero, SSD, no virtual decimation: the data part of grad_v is exactly zero (a sum of products with
    image values that are all 0), so grad_v is the regulariser half alone; a sigma FIELD as the preconditioner"""
    oc = OracleConfig(dims=DIMS, no_chains=2, data_loss='SSD', virtual_decimation=False, reg_loss=reg_loss, reg_learnable=learnable, lr=0.05)
    sigma = 0.5 + torch.rand(2, 3, *DIMS, generator=torch.Generator().manual_seed(2), dtype=F64)
    o, before, after, _, v0 = oracle64(oc, zero_moving=True, sigma=sigma)
    h = hyper_from_oracle(oc)
    y = R.reg_energy(o['curr_state'])
    assert rel(y, o['reg_energy']) < 1e-10
    sc = R.reg_scalars(y, before['reg_param'], h)
    assert rel(sc['reg_term'], o['reg']) < 1e-10
    ref = R.reg_grad_v(o['curr_state'], sc['coef'], sigma)
    gmax = float(ref.abs().max())
    assert gmax > 0 and float((ref - o['grad_v']).abs().max()) < 1e-10 * gmax
    assert float((v0 - oc.lr * ref - o['v_new']).abs().max()) < 1e-10 * float(v0.abs().max())
    assert len(sc['grads']) == (0 if not learnable else 2 if reg_loss == 'RegLoss_LogNormal' else 1)
    if learnable:
        n = len(sc['grads'])
        p, m, v = R.reg_step(sc, before['reg_param'], [0.0] * n, [0.0] * n, [0] * n, h)
        assert rel(p, after['reg_param']) < 1e-10
        assert rel(m, after['reg_m'].reshape(-1)) < 1e-10 and rel(v, after['reg_v'].reshape(-1)) < 1e-10


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU test, as far as the CPU can form them: the float32 oracle's residual and smoothed velocity
# ------------------------------------------------------------------------------------------------------------------------------
def gpu_like_inputs(dims, K, C=1):
    oc = OracleConfig(dims=dims, no_chains=C, gmm_components=K, lr=0.05)
    fixed, moving, v0, eps, unif = R.make_inputs(dims, C)
    ex = lambda d: {k: v.expand(C, *v.shape[1:]).contiguous() for k, v in d.items()}
    orc = OracleChain(oc, v0=v0)
    o = orc.transition(ex(fixed), ex(moving), eps, unif)
    ls, lg = R.hand_set_mixture(fixed, moving, K)
    state = {'log_std': ls, 'logits': lg, 'm': torch.zeros(2, K), 'v': torch.zeros(2, K), 'step': [0, 0]}
    h = hyper_from_oracle(oc)
    return o['residuals'].to(F64), fixed['mask'], o['curr_state'].to(F64), state, h


@pytest.fixture(scope='module')
def inputs_7_13_70():
    return gpu_like_inputs(DIMS, 4)


@pytest.mark.parametrize('dims,K', [((11, 13, 70), 4), ((9, 21, 67), 6)])
def test_hand_set_mixture_is_well_conditioned(dims, K):
    """a tolerance relative to S_k = sum |r_k (1 - q_k)| is vacuous if the gradient is a small difference of large sums"""
    z, mask, _, state, h = gpu_like_inputs(dims, K)
    r = R.mixture_stage(z, mask, state, h)[0][0]
    assert math.isfinite(r['alpha']) and 0.0 < r['alpha'] < 1.0
    # The data part of the log_std gradient is alpha Gs_k and its tolerance 1e-5 alpha S_k, so the ratio that must not be small is
    # |Gs_k| / S_k (0.04 .. 1.0 and 0.35 .. 1.0 here); |g_k| itself against the whole scale of its tolerance, alpha S_k + |prior
    # addend|, for both kinds of parameter (0.04 .. 1.0)
    assert bool((r['sums']['Gs'].abs() >= 0.01 * r['sums']['S']).all()), (r['sums']['Gs'], r['sums']['S'])
    assert bool((r['g'].abs() >= 0.01 * r['tol_g'] / 1e-5).all()), (r['g'], r['tol_g'])
    assert bool(torch.isfinite(r['g']).all()) and bool(torch.isfinite(r['log_std']).all())


def test_alpha_tolerance_sees_a_dropped_halo_column(inputs_7_13_70):
    z, mask, _, state, h = inputs_7_13_70
    r = R.mixture_stage(z, mask, state, h)[0][0]
    s = r['sums']
    x = s['x']
    lags = list(s['lags'])
    lags[2] -= float((x[:, :, 63] * x[:, :, 64]).sum())       # the pair that straddles the first 64-wide tile
    wrong = R.vd_alpha(s['n'], s['sxx'], lags)[0]
    assert abs(wrong - r['alpha']) >= 100.0 * R.tol_alpha(r['corr']) * r['alpha']


def test_gradient_tolerance_sees_a_missing_alpha_and_a_missing_dirichlet_term(inputs_7_13_70):
    z, mask, _, state, h = inputs_7_13_70
    r = R.mixture_stage(z, mask, state, h)[0][0]
    ls, lg = state['log_std'].to(F64), state['logits'].to(F64)
    no_alpha = R.gmm_gradients(r['sums'], 1.0, ls, lg, h)
    for i in range(2):
        assert bool(((no_alpha[i] - r['g'][i]).abs() >= 100.0 * r['tol_g'][i]).all())
    flat = R.Hyper(**{**h.__dict__, 'conc': [1.0] * h.K})         # Dir(1, ..., 1): the prior term vanishes
    no_dir = R.gmm_gradients(r['sums'], r['alpha'], ls, lg, flat)
    assert float(((no_dir[1] - r['g'][1]).abs() / r['tol_g'][1]).max()) >= 100.0
    # ... and the Adam moments the GPU test reads them through carry the same factors
    assert bool((r['tol_m'] == (1.0 - h.beta1) * r['tol_g']).all())


def test_energy_and_stencil_tolerances_see_a_single_weight_last_difference(inputs_7_13_70):
    _, _, v_s, _, h = inputs_7_13_70
    y = R.reg_energy(v_s)
    assert bool(((R.reg_energy(v_s, last_weight=1.0) - y).abs() >= 100.0 * 1e-6 * y).all())
    coef = R.reg_scalars(y, [math.log(1.4)], h)['coef']
    ref = R.reg_grad_v(v_s, coef)
    tol = R.tol_grad_v(ref, coef, v_s)
    assert float(((R.reg_grad_v(v_s, coef, last_weight=1.0) - ref).abs() / tol).max()) >= 100.0
    # a float32 evaluation of the stencil, in the update kernel's order, stays inside the bound
    assert float(((R.reg_grad_v_f32(v_s, coef).to(F64) - ref).abs() / tol).max()) <= 1.0


def test_stencil_tolerance_sees_sigma_for_sigma_squared_and_the_wrong_lognormal_coefficient(inputs_7_13_70):
    _, _, v_s, _, h = inputs_7_13_70
    sigma = 0.5 + torch.rand(v_s.shape, generator=torch.Generator().manual_seed(2), dtype=F64)
    hl = R.Hyper(**{**h.__dict__, 'reg_loss': 'RegLoss_LogNormal', 'reg_learnable': True})
    from ir_sgmcmc_amd.engine import lognormal_init
    par = lognormal_init(1.4, h.dof)
    y = R.reg_energy(v_s)
    coef = R.reg_scalars(y, par, hl)['coef']
    ref = R.reg_grad_v(v_s, coef, sigma)
    tol = R.tol_grad_v(ref, coef, v_s, sigma)
    assert float(((R.reg_grad_v_f32(v_s, coef, sigma).to(F64) - ref).abs() / tol).max()) <= 1.0
    wrong_sigma = R.reg_grad_v(v_s, coef) * sigma
    assert float(((wrong_sigma - ref).abs() / tol).max()) >= 100.0
    wrong_coef = R.reg_scalars(y, par, hl, learnable=False)['coef']
    assert float(((R.reg_grad_v(v_s, wrong_coef, sigma) - ref).abs() / tol).max()) >= 100.0
    # ... and the scalar itself against its own 1e-10 tolerance
    assert bool(((wrong_coef - coef).abs() >= 100.0 * 1e-10 * R.reg_scalars(y, par, hl)['coef_scale']).all())
