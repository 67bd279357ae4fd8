"""The torch-facing layer of the VI stage against float64, element by element: every autograd Function (SGLD, SobolevGrad, _SVFExp,
_Warp, _EnergyGrad, _LCCMap, _Energy), the RegLoss_* family and EntropyMultivariateNormal on top of them -- value and gradient, the
gradient taken with torch.autograd.grad against a random cotangent -- and the raw gradient of the first VI iteration, read from
`.grad` before Adam has normalised it.  (_FFDUp is pinned bit for bit in tests/test_gpu_ffd.py.)

The references, the inputs and the tolerances are those of tests/_autograd_modules.py: float64 autograd through the CPU oracle, and
8 E with E the deviation of the float32 CPU oracle from the float64 one on the same inputs (SGLD and the LCC map have closed forms).
tests/test_autograd_modules_host.py proves on the CPU that those tolerances see the mistakes this layer can make: sigma for sigma^2,
a missing or axis-swapped (n - 1) / 2, a swapped spacing, a dropped last plane, one chain's g_y for all, half an antithetic pair, a
factor of two.  Every record of the parity report carries E, the tolerance and the deviation."""
import copy
import json
import os

import pytest
import torch

from tests import _autograd_modules as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(t):
    return t.to(DEV).contiguous()


def ident(x):
    return 'x'.join(map(str, x)) if isinstance(x, tuple) else str(x)


def per_chain_and_expanded(im, C):
    """a (1,1,D,H,W) image as it is, .expand()-ed over the chains (stride 0) and as C contiguous copies"""
    return dev(im), dev(im).expand(C, -1, -1, -1, -1), dev(im).expand(C, -1, -1, -1, -1).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# 1  SGLD
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_sgld_value_and_gradient(dims):
    from ir_sgmcmc_amd.utils import SGLD
    c = A.sgld_case(dims)
    v, sigma, eps = (dev(c[k]).requires_grad_(True) for k in ('v', 'sigma', 'eps'))
    tau = torch.tensor(A.TAU, requires_grad=True)
    out = SGLD.apply(v, sigma, tau, eps)
    g_v, g_sigma, g_tau, g_eps = torch.autograd.grad(out, [v, sigma, tau, eps], dev(c['cot']), allow_unused=True)
    T = f'autograd/SGLD/{ident(dims)}'
    A.compare_units(T, 'value', out, c['out'], c['tol_out'])
    A.compare_units(T, 'grad_v', g_v, c['grad'], c['tol_grad'])
    assert g_sigma is None and g_tau is None and g_eps is None      # utils/functions.py:76-84


# ------------------------------------------------------------------------------------------------------------------------------
# 2  SobolevGrad
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', [1, 3])
@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_sobolev_grad_forms_agree_and_backward_is_the_identity(dims, s):
    from ir_sgmcmc_amd.utils import SobolevGrad
    c = A.sobolev_case(dims, s)
    k = torch.from_numpy(c['taps']).float()
    S = torch.stack((k, k, k)).unsqueeze(1).to(DEV)                                      # (3,1,k)
    Sd = {'x': S.unsqueeze(2).unsqueeze(2), 'y': S.unsqueeze(2).unsqueeze(4), 'z': S.unsqueeze(3).unsqueeze(4)}
    assert Sd['x'].shape == (3, 1, 1, 1, 2 * s + 1) and Sd['y'].shape == (3, 1, 1, 2 * s + 1, 1) and Sd['z'].shape == (3, 1, 2 * s + 1, 1, 1)
    cot = dev(c['cot'])
    outs = []
    for form in (Sd, k.tolist()):
        v = dev(c['v']).requires_grad_(True)
        out = SobolevGrad.apply(v, form, (s,) * 6)
        g, = torch.autograd.grad(out, v, cot)
        assert torch.equal(g, cot)
        outs.append(out.detach())
    assert torch.equal(outs[0], outs[1])
    A.compare(f'autograd/SobolevGrad/{ident(dims)}-s{s}', 'value', outs[0], A.measured(A.sobolev_oracle, dims, s)['value'])


# ------------------------------------------------------------------------------------------------------------------------------
# 3  _SVFExp through SVF_3D
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', A.SVF_MODES)
@pytest.mark.parametrize('no_steps', [4, 12])
@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_svf_exp_gradient_through_either_output(dims, no_steps, mode):
    from ir_sgmcmc_amd.utils import SVF_3D
    c, bands = A.svf_case(dims), A.svf_bands(dims, no_steps, mode)
    v = dev(c['v']).requires_grad_(True)
    t, disp = SVF_3D(dims, no_steps)(v)
    outs = {'transformation': [(t, c['g_t'])], 'displacement': [(disp, c['g_disp'])], 'both': [(t, c['g_t']), (disp, c['g_disp'])]}[mode]
    g, = torch.autograd.grad([o for o, _ in outs], v, [dev(ct) for _, ct in outs])
    T = f'autograd/SVFExp/{ident(dims)}-steps{no_steps}-{mode}'
    A.compare(T, 'transformation', t, bands['transformation'])
    A.compare(T, 'displacement [voxels]', disp, bands['displacement'])
    ratio, excluded = A.compare(T, 'grad_v', g, bands['grad_v'], cap=A.EXCLUDE_CAP)
    print(f'{T}: grad_v deviation / tolerance {ratio:.3f}, elements excluded at a cell boundary: {excluded}')


# ------------------------------------------------------------------------------------------------------------------------------
# 4  _Warp through RegistrationModule
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims', A.SHAPES, ids=ident)
def test_warp_gradient_to_the_transformation(dims):
    from ir_sgmcmc_amd.utils import RegistrationModule
    c, bands = A.warp_case(dims), A.warp_bands(dims)
    reg, cot = RegistrationModule(), dev(c['cot'])
    C = c['t'].shape[0]
    got = []
    for im in per_chain_and_expanded(c['im'], C):
        t = dev(c['t']).requires_grad_(True)
        warped = reg(im, t)
        g, = torch.autograd.grad(warped, t, cot)
        got.append((warped.detach(), g))
    im, t = dev(c['im']).requires_grad_(True), dev(c['t']).requires_grad_(True)
    reg(im, t).backward(cot)
    assert im.grad is None and torch.equal(t.grad, got[0][1])       # the moving image is data
    for warped, g in got[1:]:                                       # the stride-0 form and the per-chain form: the same bits
        assert torch.equal(warped, got[0][0]) and torch.equal(g, got[0][1])
    T = f'autograd/Warp/{ident(dims)}'
    A.compare(T, 'im_moving_warped', got[0][0], bands['warped'])
    A.compare(T, 'grad_transformation', got[0][1], bands['grad_t'])
    outside = c['outside']
    for ch in range(3):             # both faces of every axis have voxels pushed out, and the clip's zero is exact
        lo, hi = c['p'][:, ch] < 0, c['p'][:, ch] > float(c['n'][0, ch, 0, 0, 0]) - 1
        assert bool(lo.any()) and bool(hi.any())
    assert float(got[0][1].cpu()[outside].abs().max()) == 0.0
    assert float(bands['grad_t'].ref[outside].abs().max()) == 0.0 and float(bands['grad_t'].ref[~outside].abs().min()) > 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# 5  _EnergyGrad through GradientOperator
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('transformation', [False, True])
@pytest.mark.parametrize('dims', A.ENERGY_GRAD_SHAPES, ids=ident)
def test_gradient_operator_value_and_adjoint(dims, transformation):
    from ir_sgmcmc_amd.utils import GradientOperator
    c, bands = A.energy_grad_case(dims), A.energy_grad_bands(dims, transformation)
    v = dev(c['v']).requires_grad_(True)
    nabla = GradientOperator()(v, transformation=transformation)
    g, = torch.autograd.grad(nabla, v, dev(c['cot']))
    T = f'autograd/EnergyGrad/{ident(dims)}-transformation{int(transformation)}'
    A.compare(T, 'nabla', nabla, bands['nabla'])
    A.compare(T, 'grad_v', g, bands['grad_v'])


# ------------------------------------------------------------------------------------------------------------------------------
# 6  _Energy and the RegLoss_* family
# ------------------------------------------------------------------------------------------------------------------------------
def reg_module(case, dims):
    from ir_sgmcmc_amd.model import loss as L
    learn = case.endswith('learnable')
    if case.startswith('l2'):
        m = L.RegLoss_L2(A.W_REG, 'GradientOperator', list(dims), learnable=learn)
    elif case == 'student':
        m = L.RegLoss_Student('GradientOperator', list(dims))
    elif case == 'lognormal_l2':
        m = L.RegLoss_LogNormal_L2(A.W_REG, 'GradientOperator', list(dims))
    else:
        m = L.RegLoss_LogNormal(A.W_REG, 'GradientOperator', list(dims), learnable=learn)
    m = m.to(DEV)
    for name, value in A.reg_parameters(case, dims).items():        # initialised like the oracle's, then fed the oracle's bits
        p = getattr(m, name)
        assert abs(float(p.detach()) - float(value)) <= 4.0 * A.U * abs(float(value)), (name, float(p.detach()), float(value))
        with torch.no_grad():
            p.copy_(value)
        assert p.requires_grad == learn
    return m


@pytest.mark.parametrize('case', A.REG_CASES)
@pytest.mark.parametrize('dims', A.REG_SHAPES, ids=ident)
def test_regularisers_value_and_gradients_per_chain(dims, case):
    c, bands = A.reg_case(dims), A.reg_bands(case, dims)
    m = reg_module(case, dims)
    v = dev(c['v']).requires_grad_(True)
    loss, log_y = m(v)
    params = [getattr(m, k[5:]) for k in bands if k.startswith('grad_') and k != 'grad_v']
    total = (dev(c['cot_loss']) * loss).sum() + (dev(c['cot_log_y']) * log_y).sum()
    grads = torch.autograd.grad(total, [v] + params)
    T = f'autograd/Energy/{ident(dims)}-{case}'
    A.compare(T, 'loss', loss, bands['loss'])
    A.compare(T, 'log_y', log_y, bands['log_y'])
    A.compare(T, 'grad_v', grads[0], bands['grad_v'])
    for k, g in zip([k for k in bands if k.startswith('grad_') and k != 'grad_v'], grads[1:]):
        A.compare(T, k, g, bands[k])
    assert len(params) == (0 if not case.endswith('learnable') else 1 if case.startswith('l2') else 2)


# ------------------------------------------------------------------------------------------------------------------------------
# 7  _LCCMap through GMM.map
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('dims', A.LCC_SHAPES, ids=ident)
def test_lcc_map_wiring(dims, s):
    from ir_sgmcmc_amd.model.loss import GMM
    c = A.lcc_case(dims, s)
    gmm, g_z = GMM(4, s).to(DEV), dev(c['g_z'])
    C = c['moving'].shape[0]
    got = []
    for fixed in per_chain_and_expanded(c['fixed'], C):
        moving = dev(c['moving']).requires_grad_(True)
        z = gmm.map(fixed, moving)
        g, = torch.autograd.grad(z, moving, g_z)
        got.append((z.detach(), g))
    fixed, moving = dev(c['fixed']).requires_grad_(True), dev(c['moving']).requires_grad_(True)
    g, g_fixed = torch.autograd.grad(gmm.map(fixed, moving), [moving, fixed], g_z, allow_unused=True)
    assert g_fixed is None and torch.equal(g, got[0][1])            # the fixed image is data
    for z, g in got[1:]:
        assert torch.equal(z, got[0][0]) and torch.equal(g, got[0][1])
    T = f'autograd/LCCMap/{ident(dims)}-s{s}'
    A.compare_units(T, 'z', got[0][0], c['z'], c['tol_z'])
    A.compare_units(T, 'grad_moving', got[0][1], c['grad_moving'], c['tol_grad'])


# ------------------------------------------------------------------------------------------------------------------------------
# 8  EntropyMultivariateNormal
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['log_det', 'sample'])
def test_entropy_both_call_forms(form):
    from ir_sgmcmc_amd.model.loss import EntropyMultivariateNormal
    dims = A.SHAPES[0]
    c, bands = A.entropy_case(dims), A.entropy_bands(dims, form)
    names = ('log_var', 'u') if form == 'log_det' else A.ENTROPY_NAMES
    p = {k: dev(c[k]).requires_grad_(True) for k in names}
    value = EntropyMultivariateNormal()(**p)
    grads = torch.autograd.grad(value, list(p.values()), dev(c['cot']))
    T = f'autograd/EntropyMultivariateNormal/{form}'
    A.compare(T, 'value', value, bands['value'])
    for k, g in zip(p, grads):
        A.compare(T, 'grad_' + k, g, bands['grad_' + k])


# ------------------------------------------------------------------------------------------------------------------------------
# C  the gradient of the first VI iteration, before Adam
# ------------------------------------------------------------------------------------------------------------------------------
def vi_trainer(case, tmp_path):
    from ir_sgmcmc_amd.parse_config import ConfigParser
    from ir_sgmcmc_amd.trainer import Trainer
    c = A.VI_CASES[case]
    cfg = json.load(open(os.path.join(ROOT, 'configs', 'synthetic_gmm_lognormal.json')))
    cfg['trainer'].update(save_dir=str(tmp_path), no_chains=1, MCMC_init='identity', save_outputs=False)
    cfg['trainer']['uniform_noise'] = {'enabled': False, 'magnitude': 0.0}
    cfg['data_loader']['args']['dims'] = list(c['dims'])
    cfg['Sobolev_grad']['s'] = c['sobolev_s']
    cfg['virtual_decimation'] = c['vd']
    if c['reg_loss'] == 'RegLoss_L2':
        cfg['reg_loss'] = {'type': 'RegLoss_L2', 'args': {'diff_op': 'GradientOperator', 'w_reg': A.W_REG, 'learnable': c['learnable']}}
    else:
        cfg['reg_loss']['args'].update(learnable=c['learnable'], w_reg=A.W_REG)
    config = ConfigParser.from_dict(copy.deepcopy(cfg), timestamp='t')
    tm, rm = config.init_transformation_and_registration_modules()
    return Trainer(config, config.init_data_loader(), config.init_losses(), tm, rm, config.init_metrics(), device=DEV)


@pytest.mark.parametrize('case', list(A.VI_CASES))
def test_vi_gradient_before_adam(case, tmp_path):
    c, bands = A.vi_case(case), A.vi_bands(case)
    t = vi_trainer(case, tmp_path)
    fixed = {k: v.to(DEV) for k, v in c['fixed'].items()}
    moving = {k: v.to(DEV) for k, v in c['moving'].items()}
    t._engine_init(fixed, moving)
    t._GMM_init(fixed, moving, None)
    t._sobolev_init()
    t._init_optimizers()
    vp = {k: v.to(DEV).clone().requires_grad_(True) for k, v in c['vp0'].items()}
    t.optimizer_q_v = t.config.init_optimizer_q_v(vp)
    eps, x = c['eps'].to(DEV), c['x'].to(DEV)
    pert = eps * torch.exp(0.5 * vp['log_var']) + x * vp['u']          # utils/sampler.py:4-21
    t._VI_iteration(fixed, moving, vp, samples=(vp['mu'] + pert, vp['mu'] - pert))
    # zero_grad runs before backward and never after it: .grad holds this iteration's raw gradient
    T = f'autograd/VI_gradient/{case}'
    for k in A.VI_FIELDS:
        ratio = A.norm_ratio(vp[k].grad, bands['grad_' + k].ref)
        print(f'{T}: |grad_{k}| / |reference| = {ratio:.8f}')
        A.check(T, f'|grad_{k}| / |reference|', ratio, 1.0, A.NORM_RTOL)
        A.compare(T, 'grad_' + k, vp[k].grad, bands['grad_' + k])
    reg_loss = t.losses['reg']['loss']
    assert len(A.vi_param_names(case)) == sum(p.requires_grad for p in reg_loss.parameters())
    for name in A.vi_param_names(case):
        A.compare(T, 'grad_' + name, getattr(reg_loss, name).grad, bands['grad_' + name])
