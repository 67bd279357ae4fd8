"""fp64 restatement of the three stages that end a transition, each ON ITS OWN: the mixture statistics with the GMM Adam step
(trainer/trainer.py:68-77,316-327,507-514; utils/util.py:330-347,446-485), the regulariser scalars (model/loss.py:172-321;
model/distributions.py) with their Adam step (optimizers/adam_rate_decay.py:32-99), and the regulariser half of the velocity
update (utils/diff_op.py:62-96; utils/functions.py:83-84).  Plain torch, float64 throughout, no GPU, formulas written out (the
functions of oracle/ops.py pin float32 tensors in places).  Every stage takes the arrays the stage before it produced -- the
dense residual `z`, the smoothed velocity `v_s`, an energy -- so a test can feed it what the GPU itself wrote and hold the result
to rounding-level tolerances; the tolerances of tests/test_gpu_transition_scalars.py live here too (`tol_*`), so that
tests/test_transition_scalars_host.py can prove on the CPU that they see the mistakes they are for.
"""
import math
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np
import torch

F64 = torch.float64
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def f32(x):
    """a config number as the C ABI carries it (a `float` field of irs_config), as a Python double"""
    return float(np.float32(x))


@dataclass
class Hyper:
    """What the scalar stages read from the configuration (DevCfg of csrc/scalar_kernels.h), as doubles."""
    K: int = 4
    data_loss: str = 'GMM'
    virtual_decimation: bool = True
    ssd_inv_sigma: float = 10.0
    gmm_lr: Tuple[float, float] = (0.2, 0.2)          # (log_std, logits)
    gmm_lr_decay: float = 0.001
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    scale_prior: Tuple[float, float] = (0.0, 2.3)     # Normal(loc, scale) on log_std
    conc: Sequence[float] = (0.5, 0.5, 0.5, 0.5)      # Dirichlet concentration
    reg_loss: str = 'RegLoss_L2'
    reg_learnable: bool = False
    dof: float = 0.0
    reg_lr: Tuple[float, float] = (0.01, 0.01)
    reg_lr_decay: float = 0.001
    loc_prior_shape: float = 0.0                      # LogEnergyExpGammaPrior: 0.5 nu dof
    loc_prior_rate: float = 0.0                       # ... and 0.5 nu w_reg
    reg_scale_prior: Tuple[float, float] = (2.8, 5.0)
    w_reg_prior: Tuple[float, float] = (0.0, 0.0)     # LogPrecisionExpGammaPrior (shape, rate); RegLoss_Student: (a0, 2 b0)
    lr: float = 0.4


def hyper_from_engine(cfg):
    """EngineConfig -> Hyper with every `float` field of irs_config rounded to float32, as the device receives it."""
    K = cfg.gmm_components
    conc = list(cfg.dirichlet_alpha)
    conc = conc * K if len(conc) == 1 else conc[:K]
    shape = 0.5 * cfg.dof
    wprior = (float(cfg.student[0]), float(cfg.student[1])) if cfg.reg_loss == 'RegLoss_Student' else (shape, 1.0 / shape)
    w_loc = cfg.w_reg if cfg.loc_prior_w_reg is None else cfg.loc_prior_w_reg
    return Hyper(K=K, data_loss=cfg.data_loss, virtual_decimation=bool(cfg.virtual_decimation),
                 ssd_inv_sigma=float(np.float32(1.0) / np.float32(cfg.ssd_sigma)),
                 gmm_lr=(f32(cfg.gmm_lr_log_std), f32(cfg.gmm_lr_logits)), gmm_lr_decay=f32(cfg.gmm_lr_decay),
                 beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), scale_prior=(f32(cfg.scale_prior[0]), f32(cfg.scale_prior[1])),
                 conc=[f32(a) for a in conc], reg_loss=cfg.reg_loss, reg_learnable=bool(cfg.reg_learnable), dof=cfg.dof,
                 reg_lr=(f32(cfg.reg_lr[0]), f32(cfg.reg_lr[1])), reg_lr_decay=f32(cfg.reg_lr_decay),
                 loc_prior_shape=0.5 * f32(cfg.loc_prior_nu) * cfg.dof, loc_prior_rate=0.5 * f32(cfg.loc_prior_nu) * f32(w_loc),
                 reg_scale_prior=(f32(cfg.reg_scale_prior[0]), f32(cfg.reg_scale_prior[1])), w_reg_prior=wprior, lr=f32(cfg.lr))


# ------------------------------------------------------------------------------------------------------------------------------
# Adam with rate decay, one scalar or vector parameter (optimizers/adam_rate_decay.py:32-99)
# ------------------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, step, lr, decay, h: Hyper):
    """-> (p_new, m_new, v_new) in float64; clr = lr / (1 + step decay), bias corrections from step + 1."""
    clr = lr / (1.0 + step * decay)
    bc1, bc2 = 1.0 - h.beta1 ** (step + 1), 1.0 - h.beta2 ** (step + 1)
    m = h.beta1 * m + (1.0 - h.beta1) * g
    v = h.beta2 * v + (1.0 - h.beta2) * g * g
    return p - (clr / bc1) * m / (torch.sqrt(v) / math.sqrt(bc2) + h.eps), m, v


# ------------------------------------------------------------------------------------------------------------------------------
# mixture stage
# ------------------------------------------------------------------------------------------------------------------------------
def mixture_eval(z, log_std, logits, h: Hyper):
    """per element of z: (-log p(z), r (..., K), q (..., K)) with q_k = (z / sigma_k)^2 and r the responsibilities
    (model/loss.py:67-69,87-93); SSD: K = 1, r = 1, q = (z / sigma)^2, -log p = q / 2 (builder-defined)."""
    z = z.to(F64)
    if h.data_loss != 'GMM':
        q = ((z * h.ssd_inv_sigma) ** 2).unsqueeze(-1)
        return 0.5 * q[..., 0], torch.ones_like(q), q
    lp = torch.log_softmax(logits + 1e-2, dim=0)
    q = (z.unsqueeze(-1) * torch.exp(-log_std)) ** 2
    t = (lp - log_std - LOG_SQRT_2PI) - 0.5 * q
    return -torch.logsumexp(t, dim=-1), torch.softmax(t, dim=-1), q


def lag_sums(x):
    """sum x[i] x[i + 1] along D, H, W of a (D,H,W) array that is 0 off the mask (utils/util.py:446-485)"""
    return [float((x[:-1] * x[1:]).sum()), float((x[:, :-1] * x[:, 1:]).sum()), float((x[:, :, :-1] * x[:, :, 1:]).sum())]


def vd_alpha(n, sxx, lags):
    """alpha = sqrt(prod_axes min(-2/pi log corr, 1)), corr = (lag sum / n) / (sum x^2 / n); corr = 0 gives exactly 1, a negative
    one NaN like the reference.  -> (alpha, [corr_D, corr_H, corr_W])"""
    var = sxx / n
    corr = [(s / n) / var for s in lags]
    prod = 1.0
    for c in corr:
        prod *= min(-2.0 / math.pi * (math.log(c) if c > 0.0 else (-math.inf if c == 0.0 else math.nan)), 1.0)
    return math.sqrt(prod) if prod >= 0.0 else math.nan, corr


def mixture_sums(z, mask, log_std, logits, h: Hyper):
    """Everything the statistics kernel sums over one chain; z, mask: (D,H,W)."""
    nll, r, q = mixture_eval(z, log_std, logits, h)
    mk = mask.to(F64)
    x = (r * q).sum(-1) * mk
    addend = r * (1.0 - q) * mk.unsqueeze(-1)
    return {'n': float(mk.sum()), 'sxx': float((x * x).sum()), 'lags': lag_sums(x), 'x': x,
            'Gs': addend.sum((0, 1, 2)), 'S': addend.abs().sum((0, 1, 2)), 'R': (r * mk.unsqueeze(-1)).sum((0, 1, 2))}


def gmm_gradients(s, alpha, log_std, logits, h: Hyper):
    """d/d(log_std, logits) of alpha NLL - log N(log_std; loc, scale) - log Dir(log pi) in closed form, as chain_scalar_kernel
    documents them, and the sums of absolute addends behind each: -> (g_ls, g_lg, scale_ls, scale_lg, prior_ls, prior_lg)"""
    conc = torch.tensor(list(h.conc), dtype=F64)
    pi = torch.softmax(logits, dim=0)
    prior_ls = (log_std - h.scale_prior[0]) / h.scale_prior[1] ** 2
    prior_lg = -(conc - 1.0) + pi * (conc - 1.0).sum()
    g_ls = alpha * s['Gs'] + prior_ls
    g_lg = alpha * (-s['R'] + pi * s['n']) + prior_lg
    return g_ls, g_lg, s['S'], s['R'] + pi * s['n'], prior_ls, prior_lg


def tol_alpha(corr):
    """relative: 1e-5 (1 + sum_axes 1 / (2 |ln corr|)) -- a 1e-5 relative error of the sums, amplified through the logarithm"""
    amp = 0.0
    for c in corr:
        if c > 0.0:
            amp += 1.0 / (2.0 * abs(math.log(c))) if c != 1.0 else math.inf
    return 1e-5 * (1.0 + amp)


def tol_gmm_grad(alpha, scale, prior):
    """1e-5 (alpha S_k + |prior addend|): 1e-5 of the sum of the absolute addends of the gradient"""
    return 1e-5 * (abs(alpha) * scale + prior.abs())


def make_inputs(dims, C, seed=11, amp=1.5, cps=None):
    """The inputs of the GPU tests and of the host tests about them: synthetic_pair(seed=3), a starting velocity as in the variant
    tests of tests/test_gpu_transition.py (smoothed white noise, `amp` voxels) on the velocity grid, injected noise.
    -> fixed, moving (dicts of (1,1,D,H,W)), v0, eps (C,3,*dims_v), unif (C,3,*dims)"""
    from ir_sgmcmc_amd.data_loader import synthetic_pair
    from oracle import ops as O
    f1, m1 = synthetic_pair(dims, seed=3)
    fixed = {k: v.unsqueeze(0).contiguous() for k, v in f1.items() if k != 'seg'}
    moving = {k: v.unsqueeze(0).contiguous() for k, v in m1.items() if k != 'seg'}
    dv = O.control_grid_size(dims, cps) if cps else tuple(dims)
    gen = torch.Generator().manual_seed(seed)
    v0 = O.separable_conv3d_replicate(amp * torch.randn(C, 3, *dv, generator=gen), O.sobolev_kernel_1d(2, 0.5)).contiguous()
    eps = torch.randn(C, 3, *dv, generator=gen)
    unif = torch.rand(C, 3, *dims, generator=gen)
    return fixed, moving, v0, eps, unif


def hand_set_mixture(fixed, moving, K, lcc_s=1):
    """A mixture well away from its optimum, so that no gradient is a difference of nearly equal sums: the log_std of
    GMM.init_parameters (model/loss.py:61-65, from the std of the masked residual at zero velocity) shifted by +0.3, and
    logits = linspace(-0.5, 0.7, K); float32, as the device stores them.  -> (log_std, logits)"""
    from oracle import ops as O
    z = O.lcc_map(fixed['im'][:1], moving['im'][:1], lcc_s)
    sd = float(torch.std(z[fixed['mask'][:1]]))
    return (O.gmm_init_log_std(sd, K).to(torch.float32) + 0.3), torch.linspace(-0.5, 0.7, K, dtype=torch.float32)


def f32_round(p):
    return p.to(torch.float32).to(F64)


def f32_ulp(p):
    return torch.tensor(np.spacing(np.abs(p.numpy()).astype(np.float32)).astype(np.float64))


def mixture_stage(z, mask, state, h: Hyper, g_shift=0.0, round_params=True):
    """The serial recursion of api_ctx.hip over the chains of z (C,1,D,H,W) with mask (1 or C,1,D,H,W): statistics -> alpha -> one
    Adam step -> data term with the stepped parameters.  state: dict log_std, logits (K,), m, v (2,K), step (2,).
    g_shift: every gradient moved by g_shift x its tolerance (for the spread of what follows from them).
    -> (list of per-chain dicts, final state)"""
    log_std, logits = state['log_std'].to(F64).clone(), state['logits'].to(F64).clone()
    m, v, step = state['m'].to(F64).clone(), state['v'].to(F64).clone(), [int(state['step'][0]), int(state['step'][1])]
    tol_m, tol_v = torch.zeros_like(m), torch.zeros_like(v)
    out = []
    for c in range(z.shape[0]):
        zc, mc = z[c, 0], mask[c if mask.shape[0] > 1 else 0, 0]
        s = mixture_sums(zc, mc, log_std, logits, h)
        alpha, corr = vd_alpha(s['n'], s['sxx'], s['lags']) if h.virtual_decimation else (1.0, [0.0, 0.0, 0.0])
        rec = {'n': s['n'], 'alpha': alpha, 'corr': corr, 'sums': s}
        if h.data_loss == 'GMM':
            g_ls, g_lg, sc_ls, sc_lg, pr_ls, pr_lg = gmm_gradients(s, alpha, log_std, logits, h)
            t_ls, t_lg = tol_gmm_grad(alpha, sc_ls, pr_ls), tol_gmm_grad(alpha, sc_lg, pr_lg)
            g, t = torch.stack([g_ls, g_lg]), torch.stack([t_ls, t_lg])
            rec.update(g=g, tol_g=t, scale=torch.stack([sc_ls, sc_lg]))
            gs = g + g_shift * t
            # how far a gradient error within its tolerance moves the moments: the decayed sum over the chains so far
            tol_m = h.beta1 * tol_m + (1.0 - h.beta1) * t
            tol_v = h.beta2 * tol_v + (1.0 - h.beta2) * (2.0 * g.abs() * t + t * t)
            new = []
            for i in range(2):
                p, m[i], v[i] = adam_step((log_std, logits)[i], gs[i], m[i], v[i], step[i], h.gmm_lr[i], h.gmm_lr_decay, h)
                step[i] += 1
                new.append(f32_round(p) if round_params else p)
            log_std, logits = new
        rec.update(log_std=log_std.clone(), logits=logits.clone(), m=m.clone(), v=v.clone(), tol_m=tol_m.clone(), tol_v=tol_v.clone())
        rec['data_term'] = alpha * float((mixture_eval(zc, log_std, logits, h)[0] * mc.to(F64)).sum())
        out.append(rec)
    return out, {'log_std': log_std, 'logits': logits, 'm': m, 'v': v, 'step': step}


def mixture_stage_with_spread(z, mask, state, h: Hyper):
    """mixture_stage plus, per chain, `tol_param` (2,K) and `tol_data`: the spread of the stepped parameters / the data term when
    every gradient sits at + or - its tolerance, plus one float32 ulp of the parameter (the device stores it in float32)."""
    mid, final = mixture_stage(z, mask, state, h)
    lo, hi = mixture_stage(z, mask, state, h, -1.0)[0], mixture_stage(z, mask, state, h, 1.0)[0]
    for r, a, b in zip(mid, lo, hi):
        p = torch.stack([r['log_std'], r['logits']])
        spread = torch.maximum((torch.stack([a['log_std'], a['logits']]) - p).abs(), (torch.stack([b['log_std'], b['logits']]) - p).abs())
        r['tol_param'] = spread + f32_ulp(p)
        r['tol_data'] = max(abs(a['data_term'] - r['data_term']), abs(b['data_term'] - r['data_term']))
    return mid, final


# ------------------------------------------------------------------------------------------------------------------------------
# regulariser stage
# ------------------------------------------------------------------------------------------------------------------------------
def reg_energy(v, last_weight=2.0):
    """y_c = sum of the nine squared forward differences of v (C,3,D,H,W); the difference array is replicate-padded, so the last
    difference of each axis counts twice (utils/diff_op.py:78-96; model/loss.py:158-159).  `last_weight` is 2; the sensitivity
    test of the tolerances passes 1."""
    v = v.to(F64)
    y = torch.zeros(v.shape[0], dtype=F64)
    for ax in (2, 3, 4):
        n = v.shape[ax]
        d = v.narrow(ax, 1, n - 1) - v.narrow(ax, 0, n - 1)
        w = torch.ones(n - 1, dtype=F64)
        w[-1] = last_weight
        shape = [1] * 5
        shape[ax] = n - 1
        y = y + (d * d * w.view(shape)).sum((1, 2, 3, 4))
    return y


def reg_scalars(y, reg_param, h: Hyper, learnable=None):
    """Loss term, coef = d loss / d y (with the LogEnergyExpGammaPrior term when learnable) and the hyper-parameter gradients with
    their priors, per family, as functions of the energies y (C,) and the parameters; `*_scale`: sums of the absolute addends.
    -> dict reg_term, reg_term_scale, coef, coef_scale (C,), grads, grads_scale (list, one per learnable parameter)"""
    learnable = h.reg_learnable if learnable is None else learnable
    y = torch.as_tensor(y, dtype=F64)
    dof, ly = h.dof, torch.log(y)
    one = torch.ones_like(y)
    grads, gscale = [], []
    if h.reg_loss == 'RegLoss_L2':      # model/loss.py:197-198
        lw = float(reg_param[0])
        w = math.exp(lw)
        term, tscale = 0.5 * w * y - 0.5 * dof * lw, 0.5 * w * y + abs(0.5 * dof * lw)
        coef, cscale = 0.5 * w * one, 0.5 * w * one
        if learnable:                   # minus LogPrecisionExpGammaPrior(log w): d/dx [(shape - 1) x - rate e^x + x]
            shape, rate = h.w_reg_prior
            grads = [float((0.5 * w * y - 0.5 * dof).sum()) - (shape - rate * w)]
            gscale = [float((0.5 * w * y + 0.5 * dof).sum()) + shape + rate * w]
    elif h.reg_loss == 'RegLoss_Student':   # model/loss.py:234-241
        a0, b2 = h.w_reg_prior
        term = torch.log(b2 + y) * (a0 + 0.5 * dof)
        tscale = term.abs()
        coef = (a0 + 0.5 * dof) / (b2 + y)
        cscale = coef
    elif h.reg_loss == 'RegLoss_LogNormal_L2':  # model/loss.py:315-321 + :262-270
        shape, rate = 0.5 * dof, 0.5 * math.exp(float(reg_param[0]))
        parts = [-shape * math.log(rate) * one, -(shape - 1.0) * ly, rate * y, math.lgamma(shape) * one, (0.5 * dof - 1.0) * ly]
        term, tscale = sum(parts), sum(p.abs() for p in parts)
        coef, cscale = rate * one, rate * one
    else:                               # RegLoss_LogNormal, model/loss.py:266-312
        loc, ls = float(reg_param[0]), float(reg_param[1])
        sc = math.exp(ls)
        u = (ly - loc) / sc
        parts = [ly, ls * one, 0.5 * u * u, (0.5 * dof - 1.0) * ly]
        term, tscale = sum(parts), sum(p.abs() for p in parts)
        dparts = [one, u / sc, (0.5 * dof - 1.0) * one]
        if learnable:                   # minus LogEnergyExpGammaPrior at log y (trainer.py:336): -(a - 1) - 1 + b y
            dparts += [-h.loc_prior_shape * one, h.loc_prior_rate * y]
        coef, cscale = sum(dparts) / y, sum(p.abs() for p in dparts) / y
        if learnable:
            ploc, ps = h.reg_scale_prior
            grads = [float((-u / sc).sum()), float((1.0 - u * u).sum()) + (ls - ploc) / ps ** 2]
            gscale = [float((u / sc).abs().sum()), float((1.0 + u * u).sum()) + abs(ls - ploc) / ps ** 2]
    return {'reg_term': term, 'reg_term_scale': tscale, 'coef': coef, 'coef_scale': cscale, 'grads': grads, 'grads_scale': gscale}


def reg_step(sc, reg_param, adam_m, adam_v, adam_step_no, h: Hyper):
    """the Adam step on the learnable regulariser parameters -> (params, m, v), lists of doubles"""
    p, m, v = [], [], []
    for i, g in enumerate(sc['grads']):
        a, b, c = adam_step(torch.tensor(float(reg_param[i]), dtype=F64), torch.tensor(g, dtype=F64), torch.tensor(float(adam_m[i]), dtype=F64),
                            torch.tensor(float(adam_v[i]), dtype=F64), int(adam_step_no[i]), h.reg_lr[i], h.reg_lr_decay, h)
        p.append(float(a)), m.append(float(b)), v.append(float(c))
    return p, m, v


# ------------------------------------------------------------------------------------------------------------------------------
# update: the regulariser half of grad_v
# ------------------------------------------------------------------------------------------------------------------------------
def reg_grad_v(v_s, coef, sigma=None, last_weight=2.0):
    """sigma^2 2 coef D^T D v_s as autograd of sum_c coef_c y_c(v_s) in float64 (SGLD.backward: utils/functions.py:83-84)"""
    v = v_s.detach().to(F64).clone().requires_grad_(True)
    g, = torch.autograd.grad((torch.as_tensor(coef, dtype=F64) * reg_energy(v, last_weight)).sum(), v)
    return g if sigma is None else g * sigma.to(F64) ** 2


def tol_grad_v(ref, coef, v_s, sigma=None):
    """per element: sigma^2 (64 2^-24 |2 coef| max|v_s| + 2e-6 |reference|): twelve float32 differences with weights <= 2 and their sum
    (the first term, worst case), the float32 cast of 2 coef and the two products (the second).  ref is sigma^2 x the stencil."""
    s2 = 1.0 if sigma is None else sigma.to(F64) ** 2
    vmax = v_s.to(F64).abs().amax((1, 2, 3, 4)).view(-1, 1, 1, 1, 1)
    c2 = (2.0 * torch.as_tensor(coef, dtype=F64)).abs().view(-1, 1, 1, 1, 1)
    return s2 * (64.0 * 2.0 ** -24 * c2 * vmax) + 2e-6 * ref.abs()


def tol_v_new(v_in, lr, grad_v):
    """2^-23 max(|v_in|, lr |grad_v|): v_in - lr grad_v in float32, contracted into an fma or not"""
    return 2.0 ** -23 * torch.maximum(v_in.to(F64).abs(), lr * grad_v.to(F64).abs())


def reg_grad_v_f32(v_s, coef, sigma=None):
    """the stencil in float32, in the order of sgld_update_march_kernel: what the tolerance of grad_v has to leave room for"""
    v = v_s.to(torch.float32)
    lap = torch.zeros_like(v)
    for ax in (2, 3, 4):
        n = v.shape[ax]
        d = v.narrow(ax, 1, n - 1) - v.narrow(ax, 0, n - 1)
        w = torch.ones(n - 1, dtype=torch.float32)
        w[-1] = 2.0
        shape = [1] * 5
        shape[ax] = n - 1
        wd = d * w.view(shape)
        r = torch.zeros_like(v)
        r.narrow(ax, 1, n - 1).add_(wd)
        r.narrow(ax, 0, n - 1).sub_(wd)
        lap = lap + r
    c2 = (2.0 * torch.as_tensor(coef, dtype=F64)).to(torch.float32).view(-1, 1, 1, 1, 1)
    g = c2 * lap
    return g if sigma is None else sigma.to(torch.float32) ** 2 * g
